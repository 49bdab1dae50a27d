"""GPU: the trainer's optimizer path beyond plain SGD (Trainer.sgd: od_grad_stats -> od_optim_prepare -> od_optim_step_multi
-> od_copy_if_nonzero -> re-pack) against tests/optim2_ref.py, at 2 x 96^2 as test_gpu_trainer_update.py.

Updates are compared over the WHOLE flat buffers as uint32, with no tolerance: the refs are applied to a host copy of
tr.grads taken in front of each sgd(), per segment of tr.seg with the trainer's own multipliers.  The sum of squares the
norm is taken from is numpy's f64 sum here and the device's fixed-order f64 sum there; they differ in the last bits of an
f64, which the rounding to f32 in front of the square root does not keep (test_gpu_optim_exact.py checks the sum itself).

Learning rates of the functional runs (a sanity condition, not a tuned result): see FUNCTIONAL below.
"""
import numpy as np
import pytest
import torch

import ema_ref as E
import optim2_ref as R2
from test_gpu_trainer_update import B, S, _same, _setup, _step_until_sgd, _u32

pytestmark = pytest.mark.gpu

LS, WD, MOM, BETAS, EPS, DECAY = 256.0, 1e-4, 0.9, (0.9, 0.999), 1e-8, 0.99
# optimizer -> (base learning rate, clip_grad_norm) of test_functional_loss_falls: 60 steps at 8 x 96^2 from scratch with
# lr_multipliers={"h.": 1/3}, constant rate
FUNCTIONAL = {"sgd": (0.01, 10.0), "nesterov": (0.01, 10.0), "adamw": (5e-4, 10.0)}


@pytest.fixture(scope="module")
def setup():
    return _setup()


def _trainer(cuda, params, optimizer, lr, **kw):
    from object_detector_amd.trainer import Trainer
    return Trainer(params, B, (S, S), device=cuda, lr=lr, momentum=MOM, weight_decay=WD, loss_scale=LS, optimizer=optimizer,
                   betas=BETAS, adam_eps=EPS, **kw)


def _state(tr):
    from object_detector_amd import _lib
    s = _lib.OptimState.from_buffer_copy(tr.optim_state.cpu().numpy().tobytes())
    return {k: (int(s.step) if k == "step" else np.float32(getattr(s, k))) for k, _ in _lib.OptimState._fields_}


def _state_same(got, want, what, keys=None):
    for k in keys or want:
        a = np.asarray(got[k]).astype(np.float32 if k != "step" else np.int32).view(np.uint32)
        b = np.asarray(want[k]).astype(np.float32 if k != "step" else np.int32).view(np.uint32)
        assert a == b, f"{what}: {k} got {got[k]!r} want {want[k]!r}"


class Mirror:
    """Host restatement of a trainer's optimizer: the flat buffers as numpy arrays, advanced by the refs."""

    def __init__(self, tr):
        self.tr = tr
        self.w, self.m = tr.params.cpu().numpy(), tr.mom.cpu().numpy()
        self.v = None if tr.mom2 is None else tr.mom2.cpu().numpy()
        self.e = None if tr.ema is None else tr.ema.cpu().numpy()
        self.st = R2.new_state()
        self.updates = 0

    def step(self, g):
        from object_detector_amd.trainer import lr_multiplier
        tr = self.tr
        kind = R2.KINDS[tr.optimizer]
        flag, ssq = R2.grad_stats_ref(g)
        inv = np.float32(1.0 / (tr.loss_scale * tr.world))
        b1 = BETAS[0] if tr.optimizer == "adamw" else MOM
        self.st = R2.prepare_ref(self.st, ssq, flag, inv, np.float32(tr.clip_grad_norm or 0.0), b1, BETAS[1])
        omd = None if self.e is None else E.omd_ref(self.updates, tr.ema_decay, tr.ema_warmup)
        self.updates += 1
        if flag:
            return flag
        for (name, knd), (o, n) in tr.seg.items():
            sl = slice(o, o + n)
            lr = np.float32(tr.lr * lr_multiplier(name, tr.lr_multipliers))
            wd = np.float32(WD if knd == "w" else 0.0)
            nw, nm, nv = R2.step_ref(kind, self.w[sl], self.m[sl], None if self.v is None else self.v[sl], g[sl], lr, b1,
                                     BETAS[1], EPS, wd, self.st)
            self.w[sl], self.m[sl] = nw, nm
            if self.v is not None:
                self.v[sl] = nv
            if self.e is not None:
                self.e[sl] = E.ema_ref(self.e[sl], nw, omd)
        return flag

    def check(self, what):
        tr = self.tr
        _same(_u32(tr.params), self.w.view(np.uint32), f"{what}: params")
        _same(_u32(tr.mom), self.m.view(np.uint32), f"{what}: mom")
        if self.v is not None:
            _same(_u32(tr.mom2), self.v.view(np.uint32), f"{what}: mom2")
        if self.e is not None:
            _same(_u32(tr.ema), self.e.view(np.uint32), f"{what}: ema")
        _state_same(_state(tr), self.st, f"{what}: optim_state")


def _run(tr, xt, y, steps, mirror=None, what=""):
    for i in range(steps):
        _step_until_sgd(tr, xt, y)
        torch.cuda.synchronize()
        g = tr.grads.cpu().numpy()  # copied in front of sgd()
        tr.sgd()
        torch.cuda.synchronize()
        if mirror is not None:
            assert mirror.step(g) == int(tr.nonfinite.item()) == 0
            mirror.check(f"{what} step {i}")
            _same(_u32(tr.grads), g.view(np.uint32), f"{what} step {i}: gradients")


def _inputs(cuda, tr, setup):
    _params, x, anns = setup
    return torch.from_numpy(x).to(cuda), tr.pb.encode_batch(anns, return_device=True)[0]


def test_default_trainer_allocates_nothing_new(cuda, setup):
    tr = _trainer(cuda, setup[0], "sgd", 0.02)
    assert tr.mom2 is None and tr.optim_state is None and tr.last_grad_norm is None and not tr._optim_path


def test_sgd_with_idle_clipping_is_the_default_trainer(cuda, setup):
    """clip_grad_norm=1e30 takes the new path with clip_coef = 1: params and momentum after 3 steps are the default trainer's."""
    a = _trainer(cuda, setup[0], "sgd", 0.02)
    b = _trainer(cuda, setup[0], "sgd", 0.02, clip_grad_norm=1e30)
    assert b._optim_path and b.mom2 is None
    xt, y = _inputs(cuda, a, setup)
    _run(a, xt, y, 3)
    _run(b, xt, y, 3)
    _same(_u32(b.params), _u32(a.params), "params")
    _same(_u32(b.mom), _u32(a.mom), "mom")
    st = _state(b)
    assert st["step"] == 3 and st["clip_coef"] == 1.0 and st["grad_norm"] > 0 and float(b.last_grad_norm.item()) == st["grad_norm"]


@pytest.mark.parametrize("optimizer,lr", [("adamw", 1e-3), ("nesterov", 0.02)])
def test_three_steps_are_the_refs(cuda, setup, optimizer, lr):
    tr = _trainer(cuda, setup[0], optimizer, lr, ema_decay=DECAY)
    assert (tr.mom2 is not None) == (optimizer == "adamw")
    xt, y = _inputs(cuda, tr, setup)
    mir = Mirror(tr)
    _run(tr, xt, y, 3, mir, optimizer)
    assert mir.st["step"] == 3 and mir.st["clip_coef"] == 1.0
    assert np.abs(mir.w - setup_flat(tr, setup)).max() > 0


def setup_flat(tr, setup):
    host = np.zeros(tr.n_flat, np.float32)
    for (name, kind), (o, n) in tr.seg.items():
        host[o:o + n] = np.asarray(setup[0][f"{name}.{kind}"], np.float32).reshape(-1)
    return host


@pytest.mark.parametrize("optimizer,lr", [("adamw", 1e-3), ("sgd", 0.02)])
def test_clipping_engaged(cuda, setup, optimizer, lr):
    """clip_grad_norm at half of step 1's measured norm: the update is the ref's and last_grad_norm is prepare_ref's value."""
    probe = _trainer(cuda, setup[0], optimizer, lr, clip_grad_norm=1e30)
    xt, y = _inputs(cuda, probe, setup)
    _run(probe, xt, y, 1)
    norm = float(probe.last_grad_norm.item())
    assert np.isfinite(norm) and norm > 0
    tr = _trainer(cuda, setup[0], optimizer, lr, clip_grad_norm=0.5 * norm, ema_decay=DECAY)
    mir = Mirror(tr)
    _run(tr, xt, y, 1, mir, f"{optimizer} clipped")
    # the probe's gradients again: the same norm, and half of it over it (+ 1e-6) as the coefficient
    assert float(tr.last_grad_norm.item()) == float(mir.st["grad_norm"]) == norm
    assert abs(float(mir.st["clip_coef"]) - 0.5) < 1e-3
    _run(tr, xt, y, 1, mir, f"{optimizer} clipped, second")
    assert float(tr.last_grad_norm.item()) == float(mir.st["grad_norm"]) and mir.st["step"] == 2


def test_nonfinite_gradient_skips_everything(cuda, setup):
    """One Inf written into tr.grads in front of sgd(): every buffer and the bias-correction state stay, the pending flag
    is 1, and the next clean step counts step + 1."""
    tr = _trainer(cuda, setup[0], "adamw", 1e-3, clip_grad_norm=5.0, ema_decay=DECAY)
    xt, y = _inputs(cuda, tr, setup)
    mir = Mirror(tr)
    _run(tr, xt, y, 1, mir, "clean")
    keep = ("step", "b1pow", "b2pow", "bc1", "bc2")
    before = {k: t.clone() for k, t in (("params", tr.params), ("mom", tr.mom), ("mom2", tr.mom2), ("ema", tr.ema))}
    st0 = _state(tr)
    _step_until_sgd(tr, xt, y)
    tr.grads[tr.n_flat // 2] = float("inf")
    g = tr.grads.cpu().numpy()
    tr.sgd()
    torch.cuda.synchronize()
    assert mir.step(g) == 1 and int(tr.nonfinite.item()) == 1
    for k, t in before.items():
        assert torch.equal(getattr(tr, k).view(torch.int32), t.view(torch.int32)), k
    _state_same(_state(tr), st0, "skipped step", keys=keep)
    assert tr.pending_flags()[-1] == 1
    _run(tr, xt, y, 1, mir, "after the skip")  # the mirror's state did not count the skipped step either
    assert _state(tr)["step"] == st0["step"] + 1 == 2
    tr._poll_nonfinite(wait=True)
    assert tr.skipped_steps == 1


def test_state_round_trip_continues_bit_for_bit(cuda, setup, tmp_path):
    """AdamW with clipping and the average: 2 steps, state_dict -> save_state -> load_state -> a fresh trainer, 2 more
    steps == 4 uninterrupted steps.  A state of another optimizer raises; an older-format state loads into an sgd trainer."""
    from object_detector_amd import weights as W
    kw = dict(clip_grad_norm=5.0, ema_decay=DECAY)
    whole = _trainer(cuda, setup[0], "adamw", 1e-3, **kw)
    xt, y = _inputs(cuda, whole, setup)
    _run(whole, xt, y, 4)
    first = _trainer(cuda, setup[0], "adamw", 1e-3, **kw)
    _run(first, xt, y, 2)
    sd = first.state_dict()
    assert sd["optimizer"] == "adamw" and "mom2" in sd and int(sd["optim_state"]["step"]) == 2
    W.save_state(tmp_path / "state.npz", sd)
    loaded = W.load_state(tmp_path / "state.npz")
    second = _trainer(cuda, setup[0], "adamw", 1e-3, **kw)
    second.load_state_dict(loaded)
    _run(second, xt, y, 2)
    for k in ("params", "mom", "mom2", "ema", "run_stats", "optim_state"):
        _same(_u32(getattr(second, k).view(torch.float32) if k == "optim_state" else getattr(second, k)),
              _u32(getattr(whole, k).view(torch.float32) if k == "optim_state" else getattr(whole, k)), k)
    # another optimizer's state
    nest = _trainer(cuda, setup[0], "nesterov", 0.02, **kw)
    with pytest.raises(ValueError, match="optimizer"):
        nest.load_state_dict(loaded)
    # an older-format state: no "optimizer", no "mom2", no "optim_state" -> an sgd trainer takes it, an adamw one does not
    old = {k: v for k, v in loaded.items() if k not in ("optimizer", "mom2", "optim_state")}
    plain = _trainer(cuda, setup[0], "sgd", 0.02, ema_decay=DECAY)
    plain.load_state_dict(old)
    _same(_u32(plain.params), _u32(first.params), "older state: params")
    _same(_u32(plain.mom), _u32(first.mom), "older state: mom")
    with pytest.raises(ValueError, match="optimizer"):
        second.load_state_dict(old)


@pytest.mark.parametrize("optimizer", sorted(FUNCTIONAL))
def test_functional_loss_falls(cuda, optimizer):
    """60 steps on generated shapes at 96^2 with clipping: the mean total loss of the last 10 steps is below that of the
    first 10.  A sanity condition, not a tuned result."""
    import pathlib
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "scripts"))
    import _common
    import train as train_script
    from object_detector_amd import od_gen, weights as W
    from object_detector_amd.trainer import Trainer
    lr, clip = FUNCTIONAL[optimizer]
    Bf, steps = 8, 60
    X, yy = _common.shapes_dataset(32, seed=0)
    tr = Trainer(train_script.init_for_training(W.random_init(2)), Bf, (S, S), device=cuda, lr=lr, momentum=MOM,
                 weight_decay=WD, lr_multipliers={"h.": 1.0 / 3.0}, optimizer=optimizer, clip_grad_norm=clip)
    gen = od_gen.create_generator((S, S), preprocess_input=None, encode_truth=tr.pb.encode_truth_device, device=cuda,
                                  on_device=True, device_cache=True)
    batches, _ = gen.flow(X, yy, batch_size=Bf, data_augmentation=True, shuffle=True, seed=0, prefetch=2)
    lines = []
    hist = tr.fit(batches, steps, log_every=30, log=lines.append)
    batches.close()
    torch.cuda.synchronize()
    tr._poll_nonfinite(wait=True)
    first, last = float(hist[:10, 3].mean()), float(hist[-10:, 3].mean())
    print(f"{optimizer} lr {lr} clip {clip}: total loss {first:.3f} -> {last:.3f}, skipped {tr.skipped_steps}, {lines[-1]}")
    assert np.isfinite(hist).all() and last < first, (first, last)
    assert len(lines) == 2 and "grad_norm" in lines[-1]
