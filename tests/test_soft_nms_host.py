"""CPU: the numpy restatement of Soft-NMS (tests/soft_nms_ref.py) and the host side of the feature.  od_exp_neg against f64
exp, the reference's hard mode against oracle.nms on the committed golden, the conditions the generated lists of the GPU test
must meet (so that a linear / Gaussian scan that degenerates to the greedy one cannot pass it), and the config plumbing."""
import ctypes
import pathlib

import numpy as np
import pytest

import soft_nms_ref as R
from oracle import nms as onms

F = np.float32
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"


def test_exp_neg_against_f64_exp():
    """At most 2 ulp of the f32 result over [0, 80] (4e6 points and every integer), exactly 1 at 0, monotone, 0 beyond 80."""
    x = np.concatenate([np.linspace(0, 80, 4_000_001), np.arange(0, 81), np.log(2) * np.arange(0, 116)]).astype(F)
    x = np.sort(x[x <= F(80)])
    e = R.exp_neg(x)
    ref = np.exp(-x.astype(np.float64))
    ulp = np.spacing(ref.astype(F)).astype(np.float64)
    err = float(np.max(np.abs(e.astype(np.float64) - ref) / ulp))
    print(f"od_exp_neg: max error {err:.3f} ulp over {len(x)} points")
    assert err <= 2.0
    assert e.dtype == F and e[0] == F(1) and R.exp_neg(F(0)) == F(1)
    assert (np.diff(e) <= 0).all() and (e > 0).all()
    assert (R.exp_neg(np.array([np.nextafter(F(80), F(81)), 1e3, 1e30, np.inf], F)) == 0).all()


def test_hard_mode_equals_oracle_nms_on_the_golden():
    d = np.load(GOLDEN / "post_nms_64.npz")
    for b in range(2):
        for strict in (False, True):
            for max_det in (100, 5):
                keys = onms.topk_keys(d["conf"][b].reshape(-1), 256, 0.01)
                ref = onms.nms_image(d["boxes"][b], keys, 20, 0.45, strict, max_det)
                kf, kc, bx = R.soft_nms_image(d["boxes"][b], keys, 20, R.HARD, 0.45, strict, max_det, min_conf=1e-6)
                assert np.array_equal(kf, ref)
                assert np.array_equal(kc.view(np.uint32), d["conf"][b].reshape(-1)[ref].view(np.uint32))
                if not strict and max_det == 100:
                    g = d["keep"][b]
                    assert np.array_equal(kf, g[g >= 0])


@pytest.mark.parametrize("jitter", [0.01, 0.03])
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_generated_lists_tell_soft_from_hard(method, jitter):
    """Every one of the 40 generated images (the generator of tests/test_gpu_soft_nms.py) must show an emission order that is
    not ascending rank AND a kept set that differs from the greedy one; hard mode on them equals oracle.nms."""
    m = R.METHODS[method]
    for seed in range(40):
        boxes, keys = R.crowded_image(seed, jitter=jitter)
        assert len(keys) == 128 and (np.diff(keys.astype(np.int64) >> 32) <= 0).all()
        flat = (R.LOW - (keys & R.LOW)).astype(np.int64)
        rank = {int(f): i for i, f in enumerate(flat)}
        kf, kc, _ = R.soft_nms_image(boxes, keys, 3, m, R.GEN_THR, False, 200, R.GEN_SIGMA, R.GEN_MIN_CONF)
        hf, _, _ = R.soft_nms_image(boxes, keys, 3, R.HARD, R.GEN_THR, False, 200, R.GEN_SIGMA, R.GEN_MIN_CONF)
        assert np.array_equal(hf, onms.nms_image(boxes, keys, 3, R.GEN_THR, False, 200))
        r = np.array([rank[int(f)] for f in kf])
        assert (np.diff(r) < 0).any(), (method, seed, "emission order is ascending rank")
        assert set(kf.tolist()) != set(hf.tolist()), (method, seed, "kept set equals the greedy one")
        assert (np.diff(kc) <= 0).all() and (kc > F(R.GEN_MIN_CONF)).all()  # score order, all above min_conf
        assert len(set(kf.tolist())) == len(kf)


def test_crafted_lists_on_the_reference():
    """The crafted lists of the GPU test, by hand: duplicates (linear weight 0: dropped), zero-area boxes (never touched),
    a rescored tie (the lower rank wins), a chain decayed by three kept boxes."""
    for name in R.CRAFTED:
        boxes, keys, NC = R.crafted(name)
        out = {m: R.soft_nms_image(boxes, keys, NC, R.METHODS[m], 0.3, False, 200, 0.5, 0.01) for m in R.METHODS}
        n = len(keys)
        if name == "duplicates":
            assert len(out["linear"][0]) == 1 and len(out["hard"][0]) == 1
            assert len(out["gaussian"][0]) == n  # exp(-1 / sigma) > 0: decayed, kept
        elif name == "zero_area":
            for m in R.METHODS:
                assert len(out[m][0]) == n and np.array_equal(out[m][1].view(np.uint32), (keys >> np.uint64(32)).astype(np.uint32))
        elif name == "tie":
            for m in ("linear", "gaussian"):
                kf, kc, _ = out[m]
                assert len(kf) == 3 and kc[1] == kc[2] and kf[1] < kf[2]  # flat order = rank order here
        elif name == "chain":
            for m in ("linear", "gaussian"):
                kf, kc, _ = out[m]
                flat = (R.LOW - (keys & R.LOW)).astype(np.int64)
                assert len(kf) == 4 and int(kf[3]) == int(flat[3])
                s = (keys >> np.uint64(32)).astype(np.uint32).view(F)
                assert kc[3] < s[3] * F(0.6)  # (2/3)^3, or exp(-2/9)^3 = 0.51


def test_config_struct_mirrors_the_library():
    from object_detector_amd import _lib
    lib = _lib.load()
    st = _lib.SoftNmsCfg
    assert st in _lib.STRUCTS and ctypes.sizeof(st) == lib.od_sizeof(b"od_soft_nms_cfg") == 24
    buf = ctypes.create_string_buffer(256)
    n = lib.od_struct_fields(b"od_soft_nms_cfg", buf, 256)
    assert n == 6 and buf.value.decode().split(",") == [f[0] for f in st._fields_]
    for f, _ in st._fields_:
        assert getattr(st, f).offset == lib.od_offsetof(b"od_soft_nms_cfg", f.encode())
    for sym in ("od_soft_nms", "od_detect_soft", "od_tta_merge_soft", "od_slice_merge_soft"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert (_lib.OD_NMS_HARD, _lib.OD_NMS_SOFT_LINEAR, _lib.OD_NMS_SOFT_GAUSSIAN) == (R.HARD, R.LINEAR, R.GAUSSIAN)


def test_library_rejects_bad_configs_without_a_launch():
    """The OD_REQUIRE paths come before any device work: they fire with null device pointers."""
    from object_detector_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # non-null, never dereferenced

    def call(cfg, K=128):
        return lib.od_soft_nms(one, one, one, one, 1, 64, 3, K, ctypes.byref(cfg), one, one, one, None, one, 1 << 30, None)

    good = dict(method=1, strict=0, max_det=10, iou_threshold=0.3, sigma=0.5, min_conf=0.01)
    for bad, text in ((dict(method=3), "method"), (dict(method=-1), "method"), (dict(method=2, sigma=0.0), "sigma"),
                      (dict(min_conf=1e-7), "min_conf"), (dict(max_det=0), "max_det")):
        rc = call(_lib.SoftNmsCfg(**{**good, **bad}))
        assert rc != 0 and text in lib.od_last_error().decode(), (bad, lib.od_last_error())
    assert call(_lib.SoftNmsCfg(**good), K=1025) != 0 and "K <= 1024" in lib.od_last_error().decode()
    assert lib.od_soft_nms(one, one, one, one, 1, 64, 3, 128, None, one, one, one, None, one, 1 << 30, None) != 0


def test_detector_arguments_are_checked_before_the_gpu():
    """An unknown nms string, a sigma <= 0 or a min_conf below 1e-6 raise ValueError whether or not a GPU is there."""
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.postprocess import check_nms_args
    for kw in (dict(nms="soft"), dict(nms="gaussian"), dict(nms=None), dict(nms="soft-gaussian", soft_sigma=0.0),
               dict(nms="soft-linear", soft_min_conf=1e-7), dict(nms="soft-linear", soft_min_conf=-1.0)):
        with pytest.raises(ValueError):
            ObjectDetector.synthetic(1, (64, 64), **kw)
        with pytest.raises(ValueError):
            ObjectDetector({}, 1, (64, 64), **kw)
    assert check_nms_args() == ("hard", 0.5, None)
    assert check_nms_args("soft-gaussian", 0.25, 0.05) == ("soft-gaussian", 0.25, 0.05)


def test_scripts_take_the_nms_arguments():
    import argparse
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "scripts"))
    try:
        import _common
    finally:
        sys.path.pop(0)
    p = argparse.ArgumentParser()
    _common.add_nms_arguments(p)
    a = p.parse_args(["--nms", "soft-gaussian", "--soft-sigma", "0.3", "--soft-min-conf", "0.02"])
    assert (a.nms, a.soft_sigma, a.soft_min_conf) == ("soft-gaussian", 0.3, 0.02)
    assert p.parse_args([]).nms == "hard"
    with pytest.raises(SystemExit):
        p.parse_args(["--nms", "matrix"])
