"""CPU only: tests/optim_ref.py is the right optimizer, the right bf16 rounding and the right pack layout.  The GPU tests
compare the kernels with optim_ref bit for bit; this file is what ties optim_ref to something that shares none of its code."""
import numpy as np
import torch

import optim_ref as R


def test_sgd_ref_is_torch_sgd_in_float64():
    """Five steps of sgd_ref (f32, one rounding per operation) on 4096 seeded elements against torch.optim.SGD in float64:
    momentum 0.9, weight decay 1e-4, dampening 0, no Nesterov, gradient g*inv, another lr each step.
    Bound per buffer: 64 * 2**-24 * max(|w|, |m|) over the buffer -- at most 6 roundings per step for 5 steps, carried
    through a momentum recurrence whose gain is below 10 at lr <= 0.1."""
    rng = np.random.default_rng(11)
    n = 4096
    w, m = R.values(rng, n, -3, 1), np.zeros(n, np.float32)
    w0 = w.astype(np.float64)
    inv = np.float32(1.0 / 256.0)
    lrs = [0.1, 0.02, 0.05, 0.003, 0.07]
    wt = torch.tensor(w.astype(np.float64), requires_grad=True)
    opt = torch.optim.SGD([wt], lr=lrs[0], momentum=0.9, weight_decay=1e-4, dampening=0, nesterov=False)
    for lr in lrs:
        g = R.values(rng, n, -2, 3)
        w, m = R.sgd_ref(w, m, g, lr, 0.9, 1e-4, inv)
        assert w.dtype == np.float32 and m.dtype == np.float32
        for grp in opt.param_groups:
            grp["lr"] = float(np.float32(lr))
        wt.grad = torch.tensor(g.astype(np.float64) * float(inv))
        opt.step()
    w64 = wt.detach().numpy()
    m64 = opt.state[wt]["momentum_buffer"].numpy()
    bound = 64 * 2.0 ** -24 * max(np.abs(w64).max(), np.abs(m64).max())
    ew, em = np.abs(w - w64).max(), np.abs(m - m64).max()
    print(f"sgd_ref vs f64 torch SGD: |dw| {ew:.3e} |dm| {em:.3e} bound {bound:.3e}")
    assert ew <= bound and em <= bound
    assert np.abs(m64).max() > 1e-2 and np.abs(w64 - w0).max() > 1e-3  # the run moved something


def test_bf16_ref_is_torch_cpu_cast():
    rng = np.random.default_rng(0)
    big = np.array([0x7f7f8000, 0x7f7f7fff, 0xff7f8000, 0x7f7fffff], np.uint32).view(np.float32)  # around the tie to Inf
    v = np.concatenate([rng.normal(0, 1, 100000), rng.normal(0, 1e-30, 1000), rng.normal(0, 1e30, 1000),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, 1.00390625, 1.01171875, 3.3895314e38]]).astype(np.float32)
    v = np.concatenate([v, big])
    got = R.bf16_ref(v)
    want = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(v)
    assert np.array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7fc0) == 0x7fc0).all()  # NaN, quiet bit set
    one = lambda x: int(R.bf16_ref(np.array([x], np.float32))[0])
    assert one(1.00390625) == 0x3f80 and one(1.01171875) == 0x3f82  # ties: down to even, up to even
    assert one(big[0]) == 0x7f80 and one(big[1]) == 0x7f7f and one(big[2]) == 0xff80  # largest finite that rounds to Inf
    assert one(0.0) == 0 and one(-0.0) == 0x8000 and one(np.inf) == 0x7f80 and one(-np.inf) == 0xff80
    snan = np.array([0x7f800001, 0xffc00000], np.uint32).view(np.float32)
    assert list(R.bf16_ref(snan)) == [0x7fc0, 0xffc0]  # a signalling NaN with a low payload does not become Inf
    back = R.bf16_widen_ref(got)
    wb = torch.from_numpy(want.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.array_equal(back.view(np.uint32)[~nan], wb.view(np.uint32)[~nan])


def test_pack_ref_is_the_triple_loop():
    Cout, Cin, k = 16, 6, 3
    taps = k * k
    rng = np.random.default_rng(5)
    w = R.values(rng, Cout * taps * Cin, -3, 1).reshape(Cout, taps * Cin)
    cp, kp, cip, kpt = R.pack_dims(Cout, Cin, k)
    assert (cp, kp, cip, kpt) == (256, 64, 256, 192)
    wf, wt = R.pack_ref(w, Cout, Cin, k, cp, kp, cip, kpt, R.F16_NAN)
    ef, et = np.full((cp, kp), R.F16_NAN, np.uint16), np.full((cip, kpt), R.F16_NAN, np.uint16)
    for co in range(Cout):
        for tap in range(taps):
            for ci in range(Cin):
                v = np.array([w[co, tap * Cin + ci]], np.float32).astype(np.float16).view(np.uint16)[0]
                ef[co, tap * Cin + ci] = v
                et[ci, (taps - 1 - tap) * Cout + co] = v
    assert np.array_equal(wf, ef) and np.array_equal(wt, et)
    assert (wf == R.F16_NAN).sum() == cp * kp - Cout * taps * Cin and (wt == R.F16_NAN).sum() == cip * kpt - Cout * taps * Cin


def test_small_refs():
    assert R.lr_mult_ref("b.s3.0.a") == 0.01 and R.lr_mult_ref("h.out") == 1.0 / 3.0 and R.lr_mult_ref("n.lat5") == 1.0
    a = np.array([60000, np.inf, np.nan, 1.0, -0.0], np.float16)
    b = np.array([60000, -np.inf, 1.0, 2.0 ** -11, -0.0], np.float16)
    s = R.add_f16_ref(a, b)
    assert np.isposinf(s[0]) and np.isnan(s[1]) and np.isnan(s[2]) and s[3] == 1.0 and s.view(np.uint16)[4] == 0x8000
    d = np.full((1, 2, 2, 8), 30000, np.float16)
    assert np.isposinf(R.down2_ref(d)).all()  # 120000 only overflows in the sum
    d = np.array([2048, 1, 1, 1], np.float16).reshape(1, 2, 2, 1)
    assert R.down2_ref(d)[0, 0, 0, 0] == 2052  # f32 accumulation (2051), one rounding: f16 steps would stay at 2048
