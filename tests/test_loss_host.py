"""CPU: oracle/loss.py against the textbook formulas evaluated in multi-precision arithmetic, at logit margins from -200 to
+200 and gamma in {0, 0.5, 1, 2, 3}, and against finite differences for the gammas the golden test does not use.

The textbook forms (1 - p_t, log softmax as a difference, (1 - p_t)^(gamma - 1)) cancel completely in f64 at such margins;
mpmath evaluates them as written.  1 - p_t at margin 200 cancels 87 leading digits, so the working precision is 400 digits:
every reference value is good to far more than the 60 digits the comparison (rtol 1e-12) could ever see."""
import mpmath
import numpy as np
import pytest

from oracle import assign as oassign
from oracle import loss as oloss
from oracle import postprocess as opp

MARGINS = [-200.0, -100.0, -40.0, -17.0, -8.0, 0.0, 4.6, 8.0, 12.0, 17.0, 30.0, 40.0, 100.0, 200.0]
GAMMAS = [0.0, 0.5, 1.0, 2.0, 3.0]
NC = 4
DPS = 400


def _rows():
    """196 active rows (14 objectness margins x positive / background x 7 variants whose class margin walks the same list)
    and 4 ignore rows.  Margin = l_t - l_other: positive favours the right answer."""
    centres = [0.0, -3.0, 0.7, 11.0, -0.25, 5.5, -60.0]
    others = [[0.3, -0.2, 0.1], [0.0, 0.0, 0.0], [1.5, -2.0, 0.25], [-0.5, 0.5, 0.5], [3.0, 2.0, 1.0], [0.125, 0.0, -7.0],
              [-30.0, 0.0, 20.0]]
    box_d = [0.0, 0.3, -0.999, 1.0, -1.0, 2.5, -40.0]
    pred, y = [], []
    for i, d in enumerate(MARGINS):
        for pos in (True, False):
            for k in range(7):
                c = centres[k]
                lt, lo = c + d / 2, c - d / 2
                tcls = (i + k) % NC
                cm = MARGINS[(i + 2 * k + 3) % len(MARGINS)]  # true-class logit minus the largest other logit
                o = list(others[k])
                cl = o[:tcls] + [max(o) + cm] + o[tcls:]
                tb = [0.1 * k, -0.2, 0.05 * i, 1.0]
                bx = [tb[e] + box_d[(k + e) % 7] for e in range(4)]
                pred.append(([lo, lt] if pos else [lt, lo]) + cl + bx)
                onehot = [1.0 if j == tcls else 0.0 for j in range(NC)]
                y.append([0.0, 1.0] + onehot + tb if pos else [1.0, 0.0] + [0.0] * NC + [0.0] * 4)
    for k in range(4):  # ignore rows: all-zero target, arbitrary prediction
        pred.append([100.0 * k, -50.0] + [3.0 * k, 0.0, -200.0, 1.0] + [1.0, 2.0, 3.0, 4.0])
        y.append([0.0] * (NC + 6))
    return np.array(pred, np.float64), np.array(y, np.float64)


def _mp_row(p, t, alpha, gamma, box_mode):
    """Textbook loss of one row and its analytic derivative, as written, in mpmath.  -> ([obj, cls, box], grad[C])"""
    mp = mpmath.mp
    p = [mp.mpf(float(v)) for v in p]
    t = [mp.mpf(float(v)) for v in t]
    g = [mp.mpf(0)] * len(p)
    L = [mp.mpf(0)] * 3
    pos = t[1] > 0.5
    if t[0] + t[1] > 0:
        e = [mp.exp(p[0]), mp.exp(p[1])]
        sm = [e[0] / (e[0] + e[1]), e[1] / (e[0] + e[1])]
        ti = 1 if pos else 0
        pt = sm[ti]
        om = 1 - pt
        a = mp.mpf(alpha) if pos else 1 - mp.mpf(alpha)
        gm = mp.mpf(gamma)
        L[0] = -a * om ** gm * mp.log(pt)
        dl = -a * om ** gm  # d L / d log p_t
        if gamma != 0:
            dl += a * gm * om ** (gm - 1) * pt * mp.log(pt)
        for j in range(2):
            g[j] = dl * ((1 if j == ti else 0) - sm[j])
    if pos:
        ec = [mp.exp(v) for v in p[2:2 + NC]]
        s = sum(ec)
        for c in range(NC):
            q = ec[c] / s
            L[1] -= t[2 + c] * mp.log(q)
            g[2 + c] = q - t[2 + c]
        for k in range(4):
            d = p[2 + NC + k] - t[2 + NC + k]
            if box_mode == "smooth_l1":
                L[2] += d * d / 2 if abs(d) < 1 else abs(d) - mp.mpf(1) / 2
                g[2 + NC + k] = d if abs(d) < 1 else mp.sign(d)
            else:
                L[2] += d * d / 4
                g[2 + NC + k] = d / 2
    return L, g


@pytest.fixture(scope="module")
def rows():
    return _rows()


@pytest.mark.parametrize("gamma", GAMMAS)
def test_oracle_matches_multiprecision(rows, gamma):
    pred, y = rows
    assert len(pred) == 200
    alpha, mode = 0.25, "smooth_l1" if gamma != 1.0 else "mse"
    with mpmath.workdps(DPS):
        ref = [_mp_row(pred[r], y[r], alpha, gamma, mode) for r in range(len(pred))]
        ref_l = np.array([[float(v) for v in L] for L, _ in ref])
        ref_g = np.array([[float(v) for v in g] for _, g in ref])
        n = int((y[:, 1] > 0.5).sum())
        ref_sum = [float(sum(L[k] for L, _ in ref) / n) for k in range(3)]
    tol = dict(rtol=1e-12, atol=1e-300)
    # every row on its own (normaliser 1): per-component loss and every gradient element
    for r in range(len(pred)):
        l, g = oloss.loss_and_grad(pred[r:r + 1], y[r:r + 1], NC, alpha=alpha, gamma=gamma, box_mode=mode)
        assert np.isfinite(l).all() and np.isfinite(g).all(), r
        np.testing.assert_allclose(l[:3], ref_l[r], err_msg=f"row {r} {pred[r]}", **tol)
        np.testing.assert_allclose(g[0], ref_g[r], err_msg=f"row {r} {pred[r]}", **tol)
        assert l[3] == l[:3].sum()
    # all rows together: sums, normaliser = number of assigned rows, ignore rows contribute nothing
    l, g = oloss.loss_and_grad(pred, y, NC, alpha=alpha, gamma=gamma, box_mode=mode)
    assert np.isfinite(l).all() and np.isfinite(g).all()
    np.testing.assert_allclose(l[:3], ref_sum, **tol)
    np.testing.assert_allclose(g, ref_g / n, **tol)
    assert (g[-4:] == 0).all()


def test_oracle_weights_scale_components_exactly():
    pred, y = _rows()
    l1, g1 = oloss.loss_and_grad(pred, y, NC)
    l2, g2 = oloss.loss_and_grad(pred, y, NC, w=(2.0, 0.0, 0.5))
    assert (l2[:3] == l1[:3] * [2.0, 0.0, 0.5]).all()
    assert (g2[:, :2] == 2.0 * g1[:, :2]).all() and (g2[:, 2:2 + NC] == 0).all() and (g2[:, -4:] == 0.5 * g1[:, -4:]).all()


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("gamma", GAMMAS)
def test_oracle_keeps_nonfinite_input_visible(gamma, bad):
    """The contract the kernel is held to in tests/test_gpu_loss.py, restated for the oracle."""
    rng = np.random.default_rng(0)
    y = np.zeros((6, NC + 6))
    y[0, 0] = y[1, 0] = 1  # background
    y[2:5, 1] = 1  # assigned
    y[2:5, 2] = 1
    y[2:5, -4:] = rng.normal(0, 1, (3, 4))
    base = rng.normal(0, 1, y.shape)
    for r, c in [(0, 0), (1, 1), (2, 1), (3, 2), (3, 4), (4, NC + 3)]:
        pred = base.copy()
        pred[r, c] = bad
        pred[5] = bad  # ignore row
        l, g = oloss.loss_and_grad(pred, y, NC, gamma=gamma)
        assert not np.isfinite(l[3]) and not np.isfinite(g[r]).all(), (r, c)
        assert (g[5] == 0).all()
        assert np.isfinite(np.delete(g, r, 0)).all()
    pred = base.copy()
    pred[5] = bad
    l, g = oloss.loss_and_grad(pred, y, NC, gamma=gamma)
    assert np.isfinite(l).all() and np.isfinite(g).all() and (g[5] == 0).all()


@pytest.mark.parametrize("gamma", [0.0, 0.5, 3.0])
def test_loss_gradient_finite_difference_gamma(gamma):
    """tests/test_oracle_golden.py::test_loss_gradient_finite_difference, same rows, step and tolerances, other gammas."""
    rng = np.random.default_rng(0)
    pr = opp.make_priors((64, 64))
    y, a = oassign.encode_truth(np.array([[0.1, 0.1, 0.6, 0.7]], np.float32), [4], pr, 20)
    pred = rng.normal(0, 1, y.shape)
    for mode in ("smooth_l1", "mse"):
        L, g = oloss.loss_and_grad(pred, y, 20, gamma=gamma, box_mode=mode)
        rows = list(np.nonzero(a >= 0)[0][:2]) + list(np.nonzero(a == -1)[0][:1])
        for r in rows:
            for c in (0, 1, 3, 22, 25):
                p2 = pred.copy()
                p2[r, c] += 1e-6
                L2, _ = oloss.loss_and_grad(p2, y, 20, gamma=gamma, box_mode=mode)
                assert (L2[3] - L[3]) / 1e-6 == pytest.approx(g[r, c], rel=2e-3, abs=1e-7)
