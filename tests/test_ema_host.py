"""CPU: the restated weight average (tests/ema_ref.py) against float64, the decay schedule of trainer.ema_decay_at, the two
new entries of the C ABI in the header and the binding, and the training-state file of weights.save_state / load_state."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import ema_ref as E
import optim_ref as R

ROOT = pathlib.Path(__file__).resolve().parent.parent
OMDS = (0.9, 0.5, 2.0 ** -10, 1e-3, 1e-4)


@pytest.mark.parametrize("omd", OMDS, ids=str)
def test_ema_ref_is_the_float64_update_within_one_ulp(omd):
    """Within 1 f32 ulp of the result where an average lives: w within 1/8 of e.  There d = w - e is exact (Sterbenz:
    e/2 <= w <= 2e), |p| <= |e|/8 < |result|/4 so its rounding is at most 1/8 ulp of the result, and the last addition
    rounds by at most 1/2: 5/8 ulp in all.  Over unrelated e and w the result can be much smaller than d (omd near 1,
    |e| >> |w|), so there the bound is the sum of the three roundings themselves: omd * ulp(d)/2 + ulp(p)/2 + ulp(result)/2."""
    rng = np.random.default_rng(5)
    n = 1 << 16
    o32 = np.float32(omd)
    o64 = float(o32)
    e = R.values(rng, n, -3, 1)
    w = (e * (1.0 + rng.uniform(-0.125, 0.125, n))).astype(np.float32)
    got = E.ema_ref(e, w, omd)
    assert got.dtype == np.float32
    exact = e.astype(np.float64) + o64 * (w.astype(np.float64) - e.astype(np.float64))
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(exact).astype(np.float32))).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - exact) <= ulp).all()
    # unrelated values, either sign
    e, w = R.values(rng, n), R.values(rng, n)
    got = E.ema_ref(e, w, omd)
    exact = e.astype(np.float64) + o64 * (w.astype(np.float64) - e.astype(np.float64))
    d = w - e
    p = o32 * d
    bound = 0.5 * (o64 * np.spacing(np.abs(d)).astype(np.float64) + np.spacing(np.abs(p)).astype(np.float64)
                   + np.spacing(np.abs(got)).astype(np.float64))
    assert (np.abs(got.astype(np.float64) - exact) <= bound).all()
    # no intermediate is subnormal for these inputs
    tiny = np.finfo(np.float32).tiny
    nz = d != 0
    assert (np.abs(d[nz]) >= tiny).all() and (np.abs(p[nz]) >= tiny).all() and (np.abs(got[got != 0]) >= tiny).all()


def test_fixed_point_and_the_other_form():
    """w == e leaves e bit for bit, for every omd; decay * e + omd * w does not, and differs from the contract's form in the
    last bit on a large share of random inputs -- so the GPU tests can tell the two apart."""
    rng = np.random.default_rng(6)
    e = R.values(rng, 1 << 16, -3, 1)
    for omd in OMDS + (0.0, 1.0):
        assert np.array_equal(E.ema_ref(e, e.copy(), omd).view(np.uint32), e.view(np.uint32)), omd
    w = R.values(rng, e.size, -3, 1)
    for omd in (0.9, 1e-3):
        other = np.float32(1.0 - omd) * e + np.float32(omd) * w
        share = float((other.view(np.uint32) != E.ema_ref(e, w, omd).view(np.uint32)).mean())
        assert share > 0.2, (omd, share)
    kept = np.float32(0.999) * e + np.float32(1e-3) * e
    assert (kept.view(np.uint32) != e.view(np.uint32)).any()
    # omd = 0 keeps e; omd = 1 is e + (w - e) as f32 rounds it, which is not always w
    assert np.array_equal(E.ema_ref(e, w, 0.0).view(np.uint32), e.view(np.uint32))
    one = E.ema_ref(e, w, 1.0)
    assert np.array_equal(one, e + (w - e)) and (one != w).any()


def test_repeated_updates_converge_to_a_constant_w():
    rng = np.random.default_rng(7)
    w = R.values(rng, 4096, -3, 1)
    e = R.values(rng, 4096, -3, 1)
    gap0 = np.abs(e - w).max()
    for _ in range(200):
        e = E.ema_ref(e, w, 0.5)
    # 0.5 ** 200 of the first gap is left in exact arithmetic.  In f32 the average stops moving once p = d / 2 (exact) no
    # longer changes e + p, that is from |d| <= 1 ulp of e on: at most 2 ulps of w when e sits one binade above it
    assert gap0 > 1.0 and (np.abs(e - w) <= 2 * np.spacing(np.abs(w))).all()
    assert np.array_equal(E.ema_ref(w.copy(), w, 0.5), w)


def test_decay_schedule():
    from object_detector_amd import trainer as T
    for n in (0, 1, 2, 10, 100, 8990, 8991, 8992, 10 ** 6):
        for decay in (0.999, 0.99, 0.5):
            for warm in (True, False):
                assert T.ema_decay_at(n, decay, warm) == E.ema_decay_ref(n, decay, warm), (n, decay, warm)
                assert isinstance(T.ema_decay_at(n, decay, warm), float)
    got = [T.ema_decay_at(n, 0.999, True) for n in (0, 1, 10, 100)]
    assert got[0] == 0.1 and got[1] == 2.0 / 11.0 and got[2] == 0.55 and got[3] == 101.0 / 110.0
    assert [round(v, 4) for v in got] == [0.1, 0.1818, 0.55, 0.9182]
    # the ramp meets 0.999 at n = 8990 ((1 + n) / (10 + n) = 8991 / 9000) and stays there from n = 8991 on
    assert T.ema_decay_at(8989, 0.999) < 0.999 and abs(T.ema_decay_at(8990, 0.999) - 0.999) < 1e-15
    assert T.ema_decay_at(8991, 0.999) == 0.999 == T.ema_decay_at(10 ** 7, 0.999)
    assert T.ema_decay_at(0, 0.999, False) == 0.999
    # the kernel argument: 1 - decay in float64, one rounding to f32
    for n in (0, 10, 100, 8991):
        v = T.ema_omd(n, 0.999, True)
        assert isinstance(v, np.float32) and v == np.float32(1.0 - E.ema_decay_ref(n, 0.999, True)) == E.omd_ref(n, 0.999)
    assert T.ema_omd(0, 0.999) == np.float32(0.9)


def test_new_entries_are_declared_and_bound():
    """Both functions in include/odhip.h, in _lib._PROTOS with as many parameters of the same kinds, and exported."""
    from object_detector_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "odhip.h").read_text(), flags=re.S)
    want = {"od_sgd_step_multi_ema": ["ctx", "w", "m", "g", "ema", "segs", "nseg", "momentum", "inv_loss_scale",
                                      "ema_one_minus_decay", "skip_if_nonzero", "stream"],
            "od_ema_update": ["ctx", "ema", "x", "n", "one_minus_decay", "skip_if_nonzero", "stream"]}
    for name, params in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/odhip.h"
        decl = [q.strip() for q in m.group(1).split(",")]
        assert [q.split()[-1].lstrip("*") for q in decl] == params
        kinds = [C.c_void_p if "*" in q else {"int": C.c_int, "float": C.c_float, "long": C.c_longlong}[q.split()[0]]
                 for q in decl]
        assert name in _lib._PROTOS, f"{name} is missing from _lib._PROTOS"
        res, args = _lib._PROTOS[name]
        assert res is C.c_int and args == kinds, (name, args, kinds)
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(C.CDLL(str(_lib.LIB_PATH)), name), f"{name} is not exported by libodhip.so"
    assert len(_lib._PROTOS["od_sgd_step_multi"][1]) == 10  # the existing entry keeps its signature


def test_state_file_round_trip(tmp_path):
    """A hand-made state (no trainer, no GPU): every array comes back with its dtype, shape and bits -- NaN payloads, -0
    and subnormals included --, every scalar with its value, a None is left out, the file is one .npz at the path given."""
    from object_detector_amd import weights as W
    rng = np.random.default_rng(8)
    odd = np.array([0x7fc00001, 0xffc12345, 0x80000000, 0x00000001, 0x7f800000, 0x00800000], np.uint32).view(np.float32)
    sd = {"params": np.concatenate([R.values(rng, 1000), odd]), "mom": R.values(rng, 1006), "run_stats": R.values(rng, 64),
          "ema": R.values(rng, 1006), "ema_run_stats": R.values(rng, 64),
          "loss_scale": 512.0, "_good_steps": 17, "skipped_steps": 3, "_consecutive_skips": 0, "ema_updates": 123456789012,
          "ema_decay": 0.999, "step": 40,
          "layout.names": np.array(["b.conv0", "b.conv0", "h.out"]), "layout.kinds": np.array(["w", "gamma", "bias"]),
          "layout.offsets": np.array([0, 864, 900], np.int64), "layout.counts": np.array([864, 32, 106], np.int64)}
    path = tmp_path / "state.npz.tmp"  # the name the training script writes before it renames
    W.save_state(path, sd)
    assert path.exists() and sorted(p.name for p in tmp_path.iterdir()) == ["state.npz.tmp"]
    back = W.load_state(path)
    assert set(back) == set(sd)
    for k, v in sd.items():
        a = np.asarray(v)
        assert back[k].dtype == a.dtype and back[k].shape == a.shape, k
        assert back[k].tobytes() == a.tobytes(), k
    assert float(back["loss_scale"]) == 512.0 and int(back["ema_updates"]) == 123456789012 and float(back["ema_decay"]) == 0.999
    assert list(back["layout.names"]) == ["b.conv0", "b.conv0", "h.out"]
    W.save_state(path, dict(sd, ema_decay=None))
    assert "ema_decay" not in W.load_state(path)
    # numpy alone, without pickles: a file that holds an object array is refused
    np.savez(tmp_path / "pickled.npz", x=np.array([{"a": 1}], dtype=object))
    with pytest.raises(ValueError):
        W.load_state(tmp_path / "pickled.npz")


def test_train_script_parses_the_new_options(monkeypatch):
    import sys
    monkeypatch.syspath_prepend(str(ROOT / "scripts"))
    monkeypatch.setattr(sys, "argv", ["train.py"])
    import importlib
    train = importlib.import_module("train")
    p = train.build_parser()
    a = p.parse_args([])
    assert a.ema is None and a.save_state_every == 0 and a.resume is None
    a = p.parse_args(["--ema", "0.99", "--save-state-every", "20", "--resume", "results/state.npz"])
    assert a.ema == 0.99 and a.save_state_every == 20 and a.resume == pathlib.Path("results/state.npz")
    assert "NOT those an uninterrupted run" in re.sub(r"\s+", " ", p.format_help())
