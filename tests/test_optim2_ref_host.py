"""CPU only: tests/optim2_ref.py is Nesterov SGD, AdamW and clip_grad_norm_ as torch defines them.  The GPU tests compare
the kernels with optim2_ref bit for bit; this file ties optim2_ref to code that shares none of it.  The refs run in float64
here (their `dt` argument), so the only difference from torch in float64 is rounding: rtol 1e-12."""
import numpy as np
import pytest
import torch

import optim2_ref as R2
import optim_ref as R

F64 = np.float64
RTOL = 1e-12
LRS = [0.1, 0.02, 0.05, 0.003, 0.07]


def _close(a, b, what):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"{what}: max difference {err:.3e} of the largest value")
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=RTOL * np.abs(b).max(), err_msg=what)


def test_nesterov_ref_is_torch_sgd_nesterov_in_float64():
    rng = np.random.default_rng(12)
    n = 4096
    w, m = R.values(rng, n, -3, 1).astype(F64), np.zeros(n, F64)
    inv, mom, wd = 1.0 / 256.0, 0.9, 1e-4
    wt = torch.tensor(w.copy(), requires_grad=True)
    opt = torch.optim.SGD([wt], lr=LRS[0], momentum=mom, weight_decay=wd, dampening=0, nesterov=True)
    for lr in LRS:
        g = R.values(rng, n, -2, 3).astype(F64)
        w, m = R2.nesterov_ref(w, m, g, lr, mom, wd, inv, dt=F64)
        for grp in opt.param_groups:
            grp["lr"] = lr
        wt.grad = torch.tensor(g * inv)
        opt.step()
    _close(w, wt.detach().numpy(), "nesterov w")
    _close(m, opt.state[wt]["momentum_buffer"].numpy(), "nesterov m")
    assert np.abs(m).max() > 1e-2


@pytest.mark.parametrize("clip", [None, 0.05], ids=["noclip", "clip"])
def test_adamw_and_prepare_ref_are_torch_adamw_and_clip_grad_norm_in_float64(clip):
    """grad_stats_ref -> prepare_ref -> adamw_ref over 5 steps against clip_grad_norm_ + torch.optim.AdamW.  torch applies
    the decay before the Adam term (w*(1 - lr*wd) - lr*u), the ref in one expression (w - lr*(u + wd*w)): algebraically
    the same, and equal to rounding in float64."""
    rng = np.random.default_rng(13)
    n = 4096
    w, m, v = R.values(rng, n, -3, 1).astype(F64), np.zeros(n, F64), np.zeros(n, F64)
    inv, b1, b2, eps, wd = 1.0 / 256.0, 0.9, 0.999, 1e-8, 1e-2
    wt = torch.tensor(w.copy(), requires_grad=True)
    opt = torch.optim.AdamW([wt], lr=LRS[0], betas=(b1, b2), eps=eps, weight_decay=wd)
    st = {k: (x if k == "step" else F64(x)) for k, x in R2.new_state().items()}
    coefs = []
    for lr in LRS:
        g32 = R.values(rng, n, -2, 3)
        g = g32.astype(F64)
        flag, s = R2.grad_stats_ref(g32)
        st = R2.prepare_ref(st, s, flag, inv, 0.0 if clip is None else clip, b1, b2, dt=F64)
        w, m, v = R2.adamw_ref(w, m, v, g, lr, b1, b2, eps, wd, st["inv_scale_eff"], st["bc1"], st["bc2"], dt=F64)
        for grp in opt.param_groups:
            grp["lr"] = lr
        wt.grad = torch.tensor(g * inv)
        if clip is not None:
            total = torch.nn.utils.clip_grad_norm_([wt], clip)
            _close(st["grad_norm"], float(total), "grad_norm")
            coefs.append(float(st["clip_coef"]))
        opt.step()
    _close(w, wt.detach().numpy(), "adamw w")
    _close(m, opt.state[wt]["exp_avg"].numpy(), "adamw m")
    _close(v, opt.state[wt]["exp_avg_sq"].numpy(), "adamw v")
    assert st["step"] == 5 and (clip is None or max(coefs) < 1.0)  # the clipping engaged


def test_clip_coef_is_one_below_the_threshold():
    g = np.full(16, 0.25, np.float32)  # norm 1
    flag, s = R2.grad_stats_ref(g)
    st = R2.prepare_ref(R2.new_state(), s, flag, 1.0, 2.0, 0.9, 0.999)
    assert flag == 0 and float(s) == 1.0 and st["grad_norm"] == np.float32(1.0) and st["clip_coef"] == np.float32(1.0)
    wt = torch.tensor(g.astype(F64), requires_grad=True)
    wt.grad = torch.tensor(g.astype(F64))
    assert float(torch.nn.utils.clip_grad_norm_([wt], 2.0)) == 1.0 and torch.equal(wt.grad, torch.tensor(g.astype(F64)))
    st = R2.prepare_ref(R2.new_state(), s, flag, 1.0, 0.0, 0.9, 0.999)  # <= 0: no clipping
    assert st["clip_coef"] == np.float32(1.0) and st["inv_scale_eff"] == np.float32(1.0)


def test_grad_stats_ref_flags_nonfinite_and_prepare_ref_skips():
    g = np.ones(9, np.float32)
    for bad in (np.inf, -np.inf, np.nan):
        h = g.copy()
        h[4] = bad
        flag, s = R2.grad_stats_ref(h)
        assert flag == 1
        st0 = R2.prepare_ref(R2.new_state(), 9.0, 0, 1.0, 1.0, 0.9, 0.999)
        st1 = R2.prepare_ref(st0, s, flag, 1.0, 1.0, 0.9, 0.999)
        for k in ("step", "b1pow", "b2pow", "bc1", "bc2"):
            assert st1[k] == st0[k], k
    assert R2.grad_stats_ref(g) == (0, 9.0)


@pytest.mark.parametrize("beta", [0.9, 0.999])
def test_running_product_bias_correction_against_pow(beta):
    """1 - b**t from the running product against float64 pow for t <= 2000.  t rounded f32 multiplications leave the
    product within t * 2**-24 relative of b**t while it is a normal number (checked as such), and within t * 2**-149
    absolute once it is subnormal (0.9**t from t = 830: each multiplication then rounds to a multiple of 2**-149).  The
    subtraction rounds once more, so |bc - (1 - b**t)| <= t * 2**-24 * b**t + t * 2**-149 + 2**-24 * (1 - b**t): the
    t * 2**-24 bound of the multiplications, carried through the subtraction.  (Relative to 1 - b**t itself no running
    product and no powf can hold t * 2**-24 at small t: 1 - 0.999**3 cancels three digits.)  b is beta rounded to f32,
    the number the kernel multiplies by."""
    st = R2.new_state()
    b = float(np.float32(beta))
    worst = 0.0
    for t in range(1, 2001):
        st = R2.prepare_ref(st, 1.0, 0, 1.0, 0.0, beta, beta)
        exact = b ** t
        err_p = abs(float(st["b1pow"]) - exact)
        if exact >= 2.0 ** -126:
            assert err_p <= t * 2.0 ** -24 * exact, (t, err_p / exact)
        bc = 1.0 - exact
        bound = t * 2.0 ** -24 * exact + t * 2.0 ** -149 + 2.0 ** -24 * bc
        err = abs(float(st["bc1"]) - bc)
        worst = max(worst, err / bound)
        assert err <= bound, (t, err, bound)
        assert st["b1pow"].dtype == np.float32 and st["bc2"] == st["bc1"] and st["step"] == t
    print(f"beta {beta}: worst error of 1 - b**t is {worst:.3f} of its bound")


@pytest.mark.parametrize("kw", [dict(optimizer="adam"), dict(optimizer=None), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                                dict(betas=(0.9, float("nan"))), dict(betas=(0.9,)), dict(adam_eps=0.0), dict(adam_eps=-1e-8),
                                dict(adam_eps=float("inf")), dict(adam_eps=float("nan")), dict(clip_grad_norm=0.0),
                                dict(clip_grad_norm=-1.0), dict(clip_grad_norm=float("inf")),
                                dict(clip_grad_norm=float("nan"))], ids=str)
def test_trainer_rejects_bad_optimizer_arguments_before_the_device(kw, monkeypatch):
    """ValueError from the constructor with no library and no device: Context.get must not be reached."""
    from object_detector_amd import net, trainer

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(net.Context, "get", no_device)
    monkeypatch.setattr(trainer.Context, "get", no_device)
    with pytest.raises(ValueError):
        trainer.Trainer({}, 2, (96, 96), **kw)


def test_optimizer_arguments_that_are_fine():
    from object_detector_amd.trainer import check_optimizer_args
    assert check_optimizer_args("sgd", (0.9, 0.999), 1e-8, None) == ("sgd", (0.9, 0.999), 1e-8, None)
    assert check_optimizer_args("adamw", (0.0, 0.5), 1e-3, 5) == ("adamw", (0.0, 0.5), 1e-3, 5.0)
    assert check_optimizer_args("nesterov", [0.9, 0.99], 1.0, 1e30)[3] == 1e30


def test_train_script_optimizer_options():
    import pathlib
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "scripts"))
    import train
    a = train.build_parser().parse_args(["--shapes", "8"])
    assert (a.optimizer, a.beta1, a.beta2, a.adam_eps, a.clip_norm) == ("sgd", 0.9, 0.999, 1e-8, None)
    a = train.build_parser().parse_args(["--shapes", "8", "--optimizer", "adamw", "--beta1", "0.8", "--beta2", "0.99",
                                         "--adam-eps", "1e-6", "--clip-norm", "10"])
    assert (a.optimizer, a.beta1, a.beta2, a.adam_eps, a.clip_norm) == ("adamw", 0.8, 0.99, 1e-6, 10.0)
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--shapes", "8", "--optimizer", "lamb"])
