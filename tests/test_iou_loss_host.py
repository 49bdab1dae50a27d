"""CPU: the reference of the IoU-family box losses (tests/iou_loss_ref.py) on hand-computed boxes and against finite
differences, the f32-restatement tolerance and the input-validity condition of the GPU cases (test_gpu_iou_loss.py), and the
plumbing of od_loss_fwd_bwd_iou that needs no device."""
import pathlib
import re
import sys

import numpy as np
import pytest
import torch

import iou_loss_ref as R

ROOT = pathlib.Path(__file__).resolve().parent.parent
UNIT = np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)  # prior = the unit box and loc_scale 1: loc = corner offset


def _unit(b, g, mode):
    """Boxes b (predicted), g (target) given as corners -> (loss, gradient [4] w.r.t. b's corners)."""
    b, g = np.asarray(b, np.float32)[None], np.asarray(g, np.float32)[None]
    l, gr = R.loss_and_grad(b - UNIT, g - UNIT, UNIT, 1.0, mode)
    return l[0], gr[0]


# ---------------------------------------------------------------- a. hand-computed cases

@pytest.mark.parametrize("mode", list(R.MODES))
def test_identical_boxes(mode):
    for box in ([0, 0, 1, 1], [0.2, 0.3, 0.5, 0.9]):
        l, g = _unit(box, box, mode)
        assert abs(l) <= 2e-8 and np.isfinite(g).all(), (l, g)  # eps / area


def test_half_overlap():
    b, g = [0, 0, 1, 1], [0.5, 0, 1.5, 1]
    want = {"giou": 1 / 3, "diou": 1 / 3 - 0.25 / 3.25, "ciou": 1 / 3 - 0.25 / 3.25}  # same aspect ratio: v = 0
    for mode, m in want.items():
        l, _g = _unit(b, g, mode)
        assert abs((1 - l) - m) < 1e-8, (mode, 1 - l, m)


def test_disjoint_boxes_still_pull_together():
    l, g = _unit([0, 0, 1, 1], [2, 0, 3, 1], "giou")
    assert abs((1 - l) - (-1 / 3)) < 1e-8  # IoU 0, enclosing box 3 x 1, union 2
    # m = U / C - 1 with U = 2, C = 3: d m / d x2 = (dU - (U / C) dC) / C = (1 - 0) / 3, d m / d x1 = (-1 + 2 / 3) / 3.
    # Descending the loss moves b's right edge towards g (and grows b: U / C < 1 rises when both grow)
    np.testing.assert_allclose(g, [1 / 9, 0, -1 / 3, 0], atol=1e-8)
    for mode in ("diou", "ciou"):
        l, g = _unit([0, 0, 1, 1], [2, 0, 3, 1], mode)
        assert l > 1 and g[2] < 0 and g[0] + g[2] < 0, (mode, l, g)  # the centre-distance term moves the box right


@pytest.mark.parametrize("mode", list(R.MODES))
def test_crossed_corners_equal_the_sorted_box(mode):
    g = [0.25, 0.125, 1.25, 0.75]  # binary fractions: the offsets from the unit box are exact in f32
    l0, g0 = _unit([0.125, 0.25, 0.875, 1.125], g, mode)
    l1, g1 = _unit([0.875, 0.25, 0.125, 1.125], g, mode)  # x crossed
    l2, g2 = _unit([0.875, 1.125, 0.125, 0.25], g, mode)  # both crossed
    assert l0 == l1 == l2
    assert np.array_equal(g1, g0[[2, 1, 0, 3]]) and np.array_equal(g2, g0[[2, 3, 0, 1]])  # the derivative follows the selection


@pytest.mark.parametrize("mode", list(R.MODES))
def test_zero_size_predicted_box_is_finite(mode):
    for b in ([0.5, 0.5, 0.5, 0.5], [0.5, 0.1, 0.5, 0.9], [3.0, 3.0, 3.0, 3.0]):
        l, g = _unit(b, [0.2, 0.1, 0.9, 0.8], mode)
        assert np.isfinite(l) and np.isfinite(g).all() and l > 0, (b, l, g)
        l32, g32 = R.loss_and_grad_f32(np.asarray(b, np.float32)[None] - UNIT, np.float32([[0.2, 0.1, -0.1, -0.2]]), UNIT, 1.0,
                                       mode)
        assert np.isfinite(l32).all() and np.isfinite(g32).all(), (b, l32, g32)


# ---------------------------------------------------------------- b. autograd gradient = central finite differences

@pytest.mark.parametrize("mode", list(R.MODES))
def test_gradient_matches_finite_differences(mode):
    rng = np.random.default_rng(8)  # a seed whose rows keep every decision margin > 1e-4
    n, h = 50, 1e-6
    c = rng.uniform(0.1, 0.9, (n, 2))
    wh = np.exp(rng.uniform(np.log(0.03), np.log(0.9), (n, 2)))
    pr = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    yl = rng.normal(0, 1, (n, 4)).astype(np.float32)
    pl = (yl + rng.normal(0, 8.0, (n, 4))).astype(np.float32)  # some rows with crossed corners, some without overlap
    mg = R.margins(pl, yl, pr, 0.1)
    assert np.abs(mg).min() > 1e-4 and (mg[:, :2] > 0).any() and (mg[:, 6:] < 0).any()  # no kink within reach of h
    _l, g = R.loss_and_grad(pl, yl, pr, 0.1, mode)
    af = R.ciou_alpha(pl, yl, pr, 0.1) if mode == "ciou" else None  # alpha frozen at the base point
    for k in range(4):
        d = np.zeros((n, 4))
        d[:, k] = h
        fd = (R.loss_values(pl + d, yl, pr, 0.1, mode, af) - R.loss_values(pl - d, yl, pr, 0.1, mode, af)) / (2 * h)
        # central differences of an O(1) loss at h = 1e-6: truncation ~ h^2, rounding ~ 1e-16 / h
        np.testing.assert_allclose(g[:, k], fd, rtol=1e-6, atol=1e-8)


# ---------------------------------------------------------------- c. tolerance, d. input validity of the GPU cases

@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_gpu_cases_keep_their_decision_margins(regime):
    """A condition on the INPUTS: no assigned row of a GPU case sits within 1e-5 of a tie of a min / max / clamp (f32
    coordinate rounding is <= 6e-8), so f32 and f64 take the same branches and no row has to be left out."""
    priors, pos, ign, y_loc, pred_loc = R.case_rows(regime)
    mg = R.case_margins(regime)
    worst = np.abs(mg).min(0)
    print(regime, dict(zip(R.MARGIN_NAMES, worst)))
    assert mg.shape == (R.N_ASSIGNED, 8) and (np.abs(mg) >= R.MARGIN_MIN).all(), worst
    assert len(pos) == R.N_ASSIGNED and len(ign) == R.N_IGNORE and not np.intersect1d(pos, ign).size
    assert set(R.EDGE_ROWS) <= set(pos.tolist())
    w = priors[:, 2:] - priors[:, :2]
    assert (w >= 0.03 * 0.999).all() and (w <= 0.9 * 1.001).all()
    crossed = (mg[:, :2] > 0)
    print(regime, "crossed per axis", crossed.mean(), "per box", crossed.any(1).mean(), "no overlap",
          (mg[:, 6:] < 0).any(1).mean())
    if regime == "sd8":
        assert 0.1 < crossed.mean() < 0.3 and (mg[:, 6:] < 0).any()  # about 19 % per axis
    else:
        assert not crossed.any()
    for NC in (20, 75):  # the full-row cases carry exactly these loc columns
        pred, y, pr2 = R.case(regime, NC)
        assert np.array_equal(pred.reshape(-1, NC + 6)[pos, -4:], pred_loc) and pr2 is priors
        assert np.array_equal(np.nonzero(y.reshape(-1, NC + 6)[:, 1] > 0.5)[0], pos)
        assert not y.reshape(-1, NC + 6)[ign].any()


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("regime", list(R.REGIMES))
def test_f32_restatement_tolerance_is_the_recorded_one(regime, mode):
    """The f32 restatement against f64 on the very inputs of the GPU cases, as max_k |dg_k| / max_k |g_k| per row: the
    recorded constant (which the GPU test multiplies by 4) is what this measures.  giou / diou use only +, -, *, / and
    are reproducible to the bit; the 25 % headroom is for another libm's atan2 in ciou."""
    got = R.case_f32_rowrel(regime, mode)
    rec = R.F32_ROWREL_MAX[(regime, mode)]
    print(regime, mode, "measured", got, "recorded", rec)
    assert 0.5 * rec <= got <= 1.25 * rec, (got, rec)
    assert rec <= 2e-5  # the order the 200 000-row measurement found


def test_full_reference_is_the_oracle_outside_the_box_columns():
    from oracle import loss as oloss
    pred, y, priors = R.case("sd1.5", 20)
    rl, rg = R.full_reference(pred, y, priors, 20, "giou", R.LOC_SCALE, w=(2.0, 0.5, 3.0))
    ol, og = oloss.loss_and_grad(pred, y, 20, w=(2.0, 0.5, 3.0))
    assert np.array_equal(rl[:2], ol[:2]) and np.array_equal(rg[..., :-4], og[..., :-4])
    pos = y[..., 1] > 0.5
    assert (rg[~pos][:, -4:] == 0).all() and (rg[pos][:, -4:] != 0).all() and rl[2] > 0 and rl[3] == rl[:3].sum()
    _pri, prow, _ign, y_loc, pred_loc = R.case_rows("sd1.5")
    l, _g = R.loss_and_grad(pred_loc, y_loc, priors[prow % R.P], R.LOC_SCALE, "giou")
    assert rl[2] == l.sum() * 3.0 / R.N_ASSIGNED


# ---------------------------------------------------------------- e. plumbing

def test_prototype_matches_header():
    import ctypes as C
    from object_detector_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "odhip.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+od_loss_fwd_bwd_iou\s*\(([^;]*?)\)\s*;", hdr)
    assert m, "od_loss_fwd_bwd_iou is not declared in include/odhip.h"
    kinds = []
    for q in m.group(1).split(","):
        q = q.strip()
        kinds.append(C.c_void_p if "*" in q else {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}[q.split()[0]])
    res, args = _lib._PROTOS["od_loss_fwd_bwd_iou"]
    assert res is C.c_int and args == kinds, (args, kinds)
    names = [q.split()[-1].lstrip("*") for q in m.group(1).split(",")]
    assert names == ["ctx", "pred", "y", "priors", "grad", "losses", "B", "P", "NC", "focal_alpha", "focal_gamma", "box_mode",
                     "loc_scale", "w_obj", "w_cls", "w_box", "workspace", "workspace_bytes", "stream"]
    lib = _lib.load()
    assert lib.od_loss_fwd_bwd_iou.argtypes == kinds
    # od_loss_fwd_bwd keeps its signature: existing callers pass it positionally
    assert len(_lib._PROTOS["od_loss_fwd_bwd"][1]) == 17


def test_train_script_parses_the_box_loss_options(monkeypatch):
    monkeypatch.syspath_prepend(str(ROOT / "scripts"))
    sys.modules.pop("train", None)
    import train
    a = train.build_parser().parse_args(["--shapes", "8", "--box-loss", "ciou", "--box-weight", "2"])
    assert a.box_loss == "ciou" and a.box_weight == 2.0
    d = train.build_parser().parse_args([])
    assert d.box_loss == "smooth_l1" and d.box_weight == 1.0  # the default is unchanged
    for mode in ("giou", "diou", "mse"):
        assert train.build_parser().parse_args(["--box-loss", mode]).box_loss == mode
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--box-loss", "iou"])


def test_ops_reject_an_iou_mode_without_matching_priors():
    from object_detector_amd import ops
    pred = torch.zeros((2, 30, 26))
    for mode in R.MODES:
        with pytest.raises(ValueError, match="priors"):
            ops.loss_fwd_bwd(pred, pred, 20, box_mode=mode)
        with pytest.raises(ValueError, match="priors"):
            ops.loss_fwd_bwd(pred, pred, 20, box_mode=mode, priors=torch.zeros((29, 4)))
        with pytest.raises(ValueError, match="priors"):
            ops.loss_fwd_bwd(pred, pred, 20, box_mode=mode, priors=torch.zeros((30, 5)))
    with pytest.raises(ValueError, match="box_mode"):
        ops.loss_fwd_bwd(pred, pred, 20, box_mode="iou")
    assert ops.BOX_MODES == {"smooth_l1": 0, "mse": 1, **R.MODES}
