"""GPU: the trainer's weight update (Trainer.sgd: od_grad_nonfinite -> od_sgd_step_multi -> od_copy_if_nonzero ->
od_pack_weights_multi) and its host loss-scale control (Trainer._poll_nonfinite) against tests/optim_ref.py.

The update is compared over the WHOLE flat buffers as uint32, with no tolerance: the masters and the momentum after sgd() are
sgd_ref of what the buffers held right before it, per segment of tr.seg, with the learning-rate multipliers restated in
optim_ref.lr_mult_ref and weight decay on the conv weights only.  The gradients are the trainer's own (a real step at 2 x 96^2);
what is checked is the update, not them.  Learning rates stay <= 0.1; the parameters are those of weights.random_init.
"""
import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

B, S = 2, 96


def _setup(seed=2):
    from object_detector_amd import weights as W
    from object_detector_amd.pb import ObjectsAnnotation
    from oracle import network as onet
    params = W.random_init(seed)
    x = onet.synthetic_images(B, S, seed=0)
    rng = np.random.default_rng(3)
    anns = []
    for _ in range(B):
        n = int(rng.integers(1, 4))
        c = rng.uniform(0.2, 0.8, (n, 2)); wh = rng.uniform(0.15, 0.6, (n, 2))
        anns.append(ObjectsAnnotation(None, S, S, rng.integers(0, 20, n),
                                      np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)))
    return params, x, anns


@pytest.fixture(scope="module")
def setup():
    return _setup()


def _u32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"


def _step_until_sgd(tr, xt, y, inject=False):
    tr._poll_nonfinite()
    tr.forward(xt)
    tr.loss(y)
    if inject:
        tr.grad_pred[0, 5, 3] = float("inf")  # what an overflowing loss gradient looks like
    tr.backward()
    tr.allreduce()


def _checked_sgd(tr, mult, what):
    """tr.sgd() between two host copies of the flat buffers: params / mom afterwards == sgd_ref of the buffers before."""
    torch.cuda.synchronize()
    w0, m0, g0 = (t.cpu().numpy() for t in (tr.params, tr.mom, tr.grads))
    inv = np.float32(1.0 / tr.loss_scale)
    tr.sgd()
    torch.cuda.synchronize()
    covered = np.zeros(tr.n_flat, bool)
    we, me = w0.copy(), m0.copy()
    for (name, kind), (o, n) in tr.seg.items():
        covered[o:o + n] = True
        lr = np.float32(tr.lr * mult(name))
        wd = 1e-4 if kind == "w" else 0.0
        we[o:o + n], me[o:o + n] = R.sgd_ref(w0[o:o + n], m0[o:o + n], g0[o:o + n], lr, 0.9, wd, inv)
    assert int(tr.nonfinite.item()) == 0, what
    w1, m1, g1 = _u32(tr.params), _u32(tr.mom), _u32(tr.grads)
    _same(w1, we.view(np.uint32), f"{what}: params")
    _same(m1, me.view(np.uint32), f"{what}: momentum")
    _same(g1, g0.view(np.uint32), f"{what}: gradients")
    # the 0 to 3 floats behind a segment whose length is no multiple of 4 (none in this architecture: every Cout is a multiple
    # of 8; the whole-buffer comparisons above hold them to their old value in any case)
    pads = ~covered
    assert pads.sum() < 4 * len(tr.seg)
    assert not w1[pads].any() and not m1[pads].any() and not g1[pads].any(), f"{what}: a pad between segments is not +0"
    moved = sum(bool((w1[o:o + n] != w0.view(np.uint32)[o:o + n]).any()) for (o, n) in tr.seg.values())
    assert moved == len(tr.seg), f"{what}: only {moved} of {len(tr.seg)} segments moved"
    return w1.view(np.float32)


def _check_packs(tr, w, what):
    for name in ("b.s3.0.a", "b.down3", "h.out"):  # a 1x1 layer, a 3x3 stride-2 layer, the shared prediction conv (Cout = 208)
        _n, cin, cout, k, stride, _bn = tr.specs[name]
        assert (k, stride) == {"b.s3.0.a": (1, 1), "b.down3": (3, 2), "h.out": (3, 1)}[name] and (name != "h.out" or cout == 208)
        o, n = tr.seg[(name, "w")]
        dims = R.pack_dims(cout, cin, k)
        wf, wt = R.pack_ref(w[o:o + n].reshape(cout, k * k * cin), cout, cin, k, *dims, 0)
        assert tuple(tr.wf[name].shape) == dims[:2] and tuple(tr.wb[name].shape) == dims[2:]
        _same(tr.wf[name].cpu().numpy().view(np.uint16).reshape(-1), wf.reshape(-1), f"{what}: wf[{name}]")
        _same(tr.wb[name].cpu().numpy().view(np.uint16).reshape(-1), wt.reshape(-1), f"{what}: wb[{name}]")
    o, n = tr.seg[("b.conv0", "w")]
    want = np.zeros((32, 32), np.float16)
    want[:, :27] = w[o:o + n].reshape(32, 27).astype(np.float16)
    _same(tr.wf["b.conv0"].cpu().numpy().view(np.uint16).reshape(-1), want.view(np.uint16).reshape(-1), f"{what}: wf[b.conv0]")


def test_update_trajectory_is_sgd_ref(cuda, setup):
    """Four steps with momentum 0.9 and weight decay 1e-4 at lr 0.02, 0.02, 0.005, 0.013 (the device table is reused once, then
    rebuilt twice) and the loss scale changed by hand before the last one; after each sgd() the flat buffers and the f16 packs
    are the restated ones."""
    from object_detector_amd.trainer import Trainer
    params, x, anns = setup
    tr = Trainer(params, B, (S, S), device=cuda, lr=0.02, momentum=0.9, weight_decay=1e-4, loss_scale=256.0)
    xt = torch.from_numpy(x).to(cuda)
    y, _npos, _ = tr.pb.encode_batch(anns, return_device=True)
    for i, lr in enumerate((0.02, 0.02, 0.005, 0.013)):
        tr.lr = lr
        if i == 3:
            tr.loss_scale = 128.0
        _step_until_sgd(tr, xt, y)
        w = _checked_sgd(tr, R.lr_mult_ref, f"step {i}")
        _check_packs(tr, w, f"step {i}")
    assert tr.loss_scale == 128.0 and tr.skipped_steps == 0
    assert np.abs(tr.mom.cpu().numpy()).max() > 0


def test_update_with_other_multipliers(cuda, setup):
    """lr_multipliers={"h.": 0.5}: the shared layers at half the rate and the backbone at the FULL rate."""
    from object_detector_amd.trainer import Trainer
    params, x, anns = setup
    tr = Trainer(params, B, (S, S), device=cuda, lr=0.02, momentum=0.9, weight_decay=1e-4, loss_scale=256.0,
                 lr_multipliers={"h.": 0.5})
    xt = torch.from_numpy(x).to(cuda)
    y, _npos, _ = tr.pb.encode_batch(anns, return_device=True)
    _step_until_sgd(tr, xt, y)
    w = _checked_sgd(tr, lambda name: 0.5 if name.startswith("h.") else 1.0, "step 0")
    _check_packs(tr, w, "step 0")


def test_loss_scale_growth_and_skip(cuda, setup):
    """Growth interval 3: the scale doubles when the THIRD clean flag is consumed, not before; a skipped step halves it and
    resets the count of clean steps."""
    from object_detector_amd.trainer import Trainer
    params, x, anns = setup
    tr = Trainer(params, B, (S, S), device=cuda, lr=0.001, momentum=0.9, weight_decay=1e-4, loss_scale=64.0)
    tr.loss_scale_growth_interval = 3
    xt = torch.from_numpy(x).to(cuda)
    y, _npos, _ = tr.pb.encode_batch(anns, return_device=True)

    def clean_step(before, after):
        tr.step(xt, y_target=y)
        assert tr.loss_scale == before  # its own flag is still in the queue
        tr._poll_nonfinite(wait=True)
        assert int(tr.nonfinite.item()) == 0 and not tr._flag_queue
        assert tr.loss_scale == after

    clean_step(64.0, 64.0)
    clean_step(64.0, 64.0)
    clean_step(64.0, 128.0)
    assert tr.skipped_steps == 0
    p0, m0 = tr.params.clone(), tr.mom.clone()
    _step_until_sgd(tr, xt, y, inject=True)
    tr.sgd()
    assert tr.loss_scale == 128.0
    tr._poll_nonfinite(wait=True)
    assert int(tr.nonfinite.item()) == 1 and tr.skipped_steps == 1 and tr.loss_scale == 64.0
    assert torch.equal(tr.params, p0) and torch.equal(tr.mom, m0)
    clean_step(64.0, 64.0)
    clean_step(64.0, 64.0)
    clean_step(64.0, 128.0)
    assert tr.skipped_steps == 1


def _entry(value):
    """One entry of Trainer._flag_queue: a recorded event and the pinned host flag its step's copy landed in."""
    host = torch.zeros(1, dtype=torch.int32).pin_memory()
    host[0] = value
    ev = torch.cuda.Event()
    ev.record()
    return ev, host


def test_loss_scale_floor_cap_and_fixed_scale(cuda, setup):
    """_poll_nonfinite alone, on hand-made queue entries: the floor of 1.0, the cap of 65536, and dynamic_loss_scale=False."""
    from object_detector_amd.trainer import Trainer
    params, _x, _anns = setup
    tr = Trainer(params, B, (S, S), device=cuda, lr=0.001, loss_scale=2.0)
    assert tr.dynamic_loss_scale and not tr._flag_queue
    for want in (1.0, 1.0):
        tr._flag_queue.append(_entry(1))
        tr._poll_nonfinite(wait=True)
        assert tr.loss_scale == want and not tr._flag_queue
    assert tr.skipped_steps == 2 and tr._consecutive_skips == 2
    tr.loss_scale, tr.loss_scale_growth_interval = 32768.0, 1
    for want in (65536.0, 65536.0):
        tr._flag_queue.append(_entry(0))
        tr._poll_nonfinite(wait=True)
        assert tr.loss_scale == want and not tr._flag_queue
    assert tr.skipped_steps == 2 and tr._consecutive_skips == 0
    # several entries in one poll, any non-zero flag value counts as bad
    tr.loss_scale, tr.loss_scale_growth_interval = 1024.0, 2
    tr._flag_queue += [_entry(0), _entry(-1), _entry(0), _entry(0), _entry(0)]
    tr._poll_nonfinite(wait=True)
    assert tr.loss_scale == 1024.0 and tr.skipped_steps == 3 and tr._good_steps == 1  # /2 at the bad flag, x2 two clean flags later

    fx = Trainer(params, B, (S, S), device=cuda, lr=0.001, loss_scale=512.0, dynamic_loss_scale=False)
    fx.loss_scale_growth_interval = 1
    fx._flag_queue += [_entry(1), _entry(0), _entry(0), _entry(1)]
    fx._poll_nonfinite(wait=True)
    assert fx.loss_scale == 512.0 and fx.skipped_steps == 2 and not fx._flag_queue
