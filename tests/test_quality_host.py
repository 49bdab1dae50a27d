"""CPU: the reference of the quality-aware objectness terms (tests/quality_ref.py) against torch-f64 autograd of the textbook
formulas away from saturation and against multi-precision arithmetic on saturated rows (as tests/test_loss_host.py checks
oracle/loss.py), the identities that tie the soft modes to focal loss, the normalisation of the "tal" quality targets, and
every argument rule of ops / Trainer that needs no device."""
import pathlib
import re
import sys

import mpmath
import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))

import quality_ref as qr  # noqa: E402
from oracle import loss as oloss  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent
GAMMAS = [1.0, 2.0, 3.0]
ALPHA = 0.25


def _rows(zs, qs):
    """one assigned row per (z, q), one background row per z, two ignore rows -> (pred [R,2], y [R,2], quality [R])"""
    pred, y, q = [], [], []
    for i, z in enumerate(zs):
        c = 0.3 * (i % 5) - 0.6
        for v in qs:
            pred.append([c - z / 2, c + z / 2]), y.append([0.0, 1.0]), q.append(v)
        pred.append([c - z / 2, c + z / 2]), y.append([1.0, 0.0]), q.append(0.7)  # quality of a background row is not read
    for z in (3.0, -50.0):
        pred.append([0.0, z]), y.append([0.0, 0.0]), q.append(0.5)
    return np.array(pred), np.array(y), np.array(q)


def _textbook_torch(pred, y, q, mode, gamma):
    """L per row from the published formulas, d L / d z by autograd (f64)"""
    z = torch.tensor(pred[:, 1] - pred[:, 0], requires_grad=True)
    qt = torch.tensor(q)
    pos, act = torch.tensor(y[:, 1] > 0.5), torch.tensor(y.sum(1) > 0)
    p = torch.sigmoid(z)
    bce = -(qt * torch.log(p) + (1 - qt) * torch.log(1 - p))
    bg = -(1 - ALPHA) * p ** gamma * torch.log(1 - p)
    if mode == "qfl":
        soft = ALPHA * torch.abs(qt - p) ** gamma * bce
        L = torch.where(pos, soft, bg)
    else:
        L = torch.where(pos & (qt > 0), qt * bce, bg)
    L = torch.where(act, L, torch.zeros_like(L))
    L.sum().backward()
    return L.detach().numpy(), z.grad.numpy()


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("mode", ["qfl", "vfl"])
def test_reference_matches_autograd_of_the_textbook_formula(mode, gamma):
    zs = np.linspace(-7.5, 7.5, 31) + 0.013
    pred, y, q = _rows(zs, [0.0, 1e-6, 0.11, 0.5, 0.83, 1.0])
    L, g, p = qr.objectness(pred, y, q, mode, ALPHA, gamma)
    pos = y[:, 1] > 0.5
    assert np.abs(q - p)[pos].min() > 1e-4  # away from the kink of |q - p| at gamma = 1
    Lt, gt = _textbook_torch(pred, y, q, mode, gamma)
    np.testing.assert_allclose(L, Lt, rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose(g, gt, rtol=1e-9, atol=1e-300)
    assert (L[-2:] == 0).all() and (g[-2:] == 0).all()


def _mp_row(z, q, pos, mode, gamma):
    mp = mpmath.mp
    z, q, a, gm = mp.mpf(float(z)), mp.mpf(float(q)), mp.mpf(ALPHA), mp.mpf(gamma)
    p = 1 / (1 + mp.exp(-z))
    bce = -(q * mp.log(p) + (1 - q) * mp.log(1 - p))
    if not pos or (mode == "vfl" and q == 0):
        L = -(1 - a) * p ** gm * mp.log(1 - p)
        g = (1 - a) * (p ** gm * p - gm * p ** (gm - 1) * p * (1 - p) * mp.log(1 - p))
        return L, g
    if mode == "vfl":
        return q * bce, q * (p - q)
    d = abs(p - q)
    return a * d ** gm * bce, a * (gm * d ** (gm - 1) * mp.sign(p - q) * p * (1 - p) * bce + d ** gm * (p - q))


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("mode", ["qfl", "vfl"])
def test_reference_matches_multiprecision_on_saturated_rows(mode, gamma):
    """margins to +-200: the textbook 1 - p and p - q cancel completely in f64 there; 400 digits evaluate them as written"""
    zs = [-200.0, -100.0, -40.0, -17.0, -8.0, 0.0, 4.6, 8.0, 12.0, 17.0, 30.0, 40.0, 100.0, 200.0]
    pred, y, q = _rows(zs, [0.0, 1e-6, 0.25, 0.5, 1.0])
    L, g, _p = qr.objectness(pred, y, q, mode, ALPHA, gamma)
    assert np.isfinite(L).all() and np.isfinite(g).all()
    with mpmath.workdps(400):
        ref = [_mp_row(pred[r, 1] - pred[r, 0], q[r], y[r, 1] > 0.5, mode, gamma) if y[r].sum() > 0 else (0, 0)
               for r in range(len(pred))]
        Lr, gr = np.array([float(v[0]) for v in ref]), np.array([float(v[1]) for v in ref])
    np.testing.assert_allclose(L, Lr, rtol=1e-12, atol=1e-300)
    # q = 0.25 / 0.5 against a saturated p: p - q is a well-conditioned difference; everything else has no difference at all
    np.testing.assert_allclose(g, gr, rtol=1e-12, atol=1e-300)


def _loss_case(seed=0, R=400, NC=5):
    rng = np.random.default_rng(seed)
    y = np.zeros((R, NC + 6))
    y[:, 0] = 1
    pos = np.sort(rng.permutation(R)[:60])
    y[pos, 0], y[pos, 1] = 0, 1
    y[pos, 2 + rng.integers(0, NC, len(pos))] = 1
    y[pos, -4:] = rng.normal(0, 1, (len(pos), 4))
    y[rng.permutation(np.setdiff1d(np.arange(R), pos))[:30]] = 0
    pred = rng.normal(0, 3, y.shape)
    return pred.astype(np.float32), y.astype(np.float32), pos


@pytest.mark.parametrize("gamma", GAMMAS)
def test_qfl_with_quality_one_is_focal(gamma):
    pred, y, _pos = _loss_case()
    q = np.ones(len(pred))
    rl, rg = qr.loss_and_grad(pred, y, q, 5, "qfl", gamma=gamma)
    fl, fg = oloss.loss_and_grad(pred, y, 5, gamma=gamma)
    np.testing.assert_allclose(rl, fl, rtol=1e-12)
    np.testing.assert_allclose(rg, fg, rtol=1e-11, atol=1e-300)
    # and mode "focal" of the reference IS the oracle
    zl, zg = qr.loss_and_grad(pred, y, None, 5, "focal", gamma=gamma)
    np.testing.assert_allclose(zl, fl, rtol=1e-14)
    np.testing.assert_allclose(zg, fg, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("mode", ["qfl", "vfl"])
def test_background_rows_are_focal(mode):
    pred, y, pos = _loss_case(1)
    q = np.random.default_rng(2).uniform(0, 1, len(pred))
    q[pos[:3]] = [0.0, np.nan, -4.0]  # NaN and negative values clamp to 0
    _rl, rg = qr.loss_and_grad(pred, y, q, 5, mode)
    _fl, fg = oloss.loss_and_grad(pred, y, 5)
    bg = y[:, 1] < 0.5
    # two f64 spellings of one term (p as {1, e} / (1 + e) here, as exp(log p) in oracle/loss.py): equal to rounding; the
    # DEVICE's background columns are compared bit for bit in test_gpu_quality.py
    np.testing.assert_allclose(rg[bg], fg[bg], rtol=1e-13, atol=0)
    assert np.abs(fg[bg, :2]).max() > 0
    assert np.array_equal(rg[:, 2:], fg[:, 2:])  # class and box columns untouched
    assert not np.array_equal(rg[pos, :2], fg[pos, :2])
    if mode == "vfl":  # q == 0 on an assigned row: focal's background term, as published
        L, g, p = qr.objectness(pred, y, q, mode)
        yb = y.copy()
        yb[pos[:3], 0], yb[pos[:3], 1] = 1, 0
        Lb, gb, _ = qr.objectness(pred, yb, q, "focal")
        assert np.array_equal(L[pos[:3]], Lb[pos[:3]]) and np.array_equal(g[pos[:3]], gb[pos[:3]])


def test_tal_normalisation_gives_each_object_its_best_iou():
    """per object: max q over its aligned rows == umax, bit for bit (the row of the largest l carries expf(0) * umax); forced
    rows carry max(u, static IoU); nothing else is nonzero"""
    import tal_cases as tc
    from object_detector_amd import priors as PR
    case = ((64, 64), (4, 20, 7), 13, False)
    anns, pred, refs, shown = tc.reference(case)
    assert "forced" in shown
    pri = PR.make_priors(case[0])
    B, G = len(anns), case[1][2]
    gb = np.zeros((B, G, 4), np.float32)
    for i, a in enumerate(anns):
        gb[i, :a.num_objects] = a.bboxes
    y = np.stack([r["y"] for r in refs])
    assigned = np.stack([r["assigned"] for r in refs])
    metric = np.stack([r["metric"] for r in refs]).astype(np.float32)
    out = qr.quality_tal(pred, y, pri, gb, assigned, metric)
    q = out["q"]
    assert out["aligned"].sum() > 50 and out["forced"].sum() >= 2
    assert ((q >= 0) & (q <= 1)).all() and (q[~(out["aligned"] | out["forced"])] == 0).all()
    seen = 0
    for b in range(B):
        for g in range(G):
            m = out["aligned"][b] & (assigned[b] == g)
            if m.any():
                assert q[b, m].max() == np.float64(out["umax"][b, g]) == np.float64(out["u"][b, m].max())
                assert (q[b, m] <= q[b, m].max()).all()
                seen += 1
    assert seen >= 5
    assert (out["exact"] | out["aligned"]).all() and (out["dl"] <= 0).all()
    # the same rows through the "iou" mode: the decoded target of a row is (up to the encode's rounding) its object's box
    qi = qr.quality_iou(pred, y, pri)
    pos = y[..., 1] > 0.5
    assert (qi[~pos] == 0).all() and np.abs(qi[pos] - out["u"][pos]).max() < 1e-4


def test_quality_is_clamped_and_nan_is_zero():
    assert np.array_equal(qr.clamp_quality([-1.0, 0.0, 0.5, 1.0, 7.0, np.nan, np.inf]), [0, 0, 0.5, 1, 1, 0, 1])


# ---------------------------------------------------------------- argument rules (no device)

def test_ops_argument_rules():
    from object_detector_amd import ops
    pred = torch.zeros((2, 10, 9))
    y = torch.zeros((2, 10, 9))
    pri = torch.zeros((10, 4))
    q = torch.zeros((2, 10))
    with pytest.raises(ValueError, match="objectness must be one of"):
        ops.loss_fwd_bwd(pred, y, 3, objectness="gfl", quality=q)
    for mode in ("qfl", "vfl"):
        with pytest.raises(ValueError, match="needs quality"):
            ops.loss_fwd_bwd(pred, y, 3, objectness=mode)
        for bad in (q[:1], q[:, :-1], torch.zeros((2, 10, 1)), torch.zeros((20,))):
            with pytest.raises(ValueError, match="does not match"):
                ops.loss_fwd_bwd(pred, y, 3, objectness=mode, quality=bad)
    for g in (0.5, 0.0, 0.999, float("nan")):
        with pytest.raises(ValueError, match="gamma >= 1"):
            ops.loss_fwd_bwd(pred, y, 3, gamma=g, objectness="qfl", quality=q)
    ops.check_objectness("vfl", q, 0.5, pred.shape[:-1])  # varifocal has no |q - p|^gamma on the assigned rows
    ops.check_objectness("focal", None, 0.0, pred.shape[:-1])
    with pytest.raises(ValueError, match="box_mode"):  # the box rules still come first
        ops.loss_fwd_bwd(pred, y, 3, box_mode="iou", objectness="qfl", quality=q)
    with pytest.raises(ValueError, match="quality mode must be one of"):
        ops.quality_targets(pred, y, pri, mode="giou")
    a, m, gb = torch.zeros((2, 10), dtype=torch.int32), torch.zeros((2, 10)), torch.zeros((2, 3, 4))
    for kw in (dict(), dict(assigned=a), dict(assigned=a, metric=m), dict(metric=m, gt_boxes=gb), dict(assigned=a, gt_boxes=gb)):
        with pytest.raises(ValueError, match='"tal" needs'):
            ops.quality_targets(pred, y, pri, mode="tal", **kw)
    ops.check_quality_mode("tal", a, m, gb)
    ops.check_quality_mode("iou")
    assert ops.OBJ_MODES == {"focal": 0, "qfl": 1, "vfl": 2}


def test_trainer_argument_rules(monkeypatch):
    """every rule fails in the constructor before the device is touched"""
    from object_detector_amd import trainer as T

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(T.Context, "get", no_device)
    with pytest.raises(ValueError, match="objectness must be one of"):
        T.Trainer({}, 2, objectness="gfl")
    with pytest.raises(ValueError, match="quality must be one of"):
        T.Trainer({}, 2, objectness="qfl", quality="giou")
    for assigner in ("max-iou", "atss"):
        for obj in ("focal", "qfl", "vfl"):
            with pytest.raises(ValueError, match='needs assigner="tal"'):
                T.Trainer({}, 2, objectness=obj, quality="tal", assigner=assigner)
    for obj in ("focal", "qfl", "vfl"):  # these pass the checks and go on to the device
        with pytest.raises(AssertionError, match="the device was touched"):
            T.Trainer({}, 2, objectness=obj, quality="tal", assigner="tal")
        with pytest.raises(AssertionError, match="the device was touched"):
            T.Trainer({}, 2, objectness=obj, quality="iou", assigner="atss")


def test_train_script_has_the_options():
    sys.path.insert(0, str(ROOT / "scripts"))
    import train as train_script
    p = train_script.build_parser()
    a = p.parse_args(["--vocdevkit-dir", "x"] if any(ac.dest == "vocdevkit_dir" and ac.required for ac in p._actions) else [])
    assert (a.objectness, a.quality) == ("focal", "iou")
    argv = [s for s in sys.argv]
    b = p.parse_args(["--objectness", "qfl", "--quality", "tal"])
    assert (b.objectness, b.quality) == ("qfl", "tal") and sys.argv == argv
    with pytest.raises(SystemExit):
        p.parse_args(["--objectness", "gfl"])


def test_header_and_binding_declare_the_entries():
    from object_detector_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "odhip.h").read_text(), flags=re.S)
    for name in ("od_loss_fwd_bwd_quality", "od_quality_iou", "od_quality_tal", "od_quality_tal_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib._PROTOS
    lib = _lib.load()
    assert lib.od_quality_tal_workspace_bytes(3, 7) == 3 * 7 * 8 and lib.od_quality_tal_workspace_bytes(0, 7) == 0
