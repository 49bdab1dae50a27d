"""GPU parity of od_augment_warp (K14b: affine warp + colour matrix + MixUp of mosaic frames) against tests/warp_ref.py, bit for
bit and without excluded pixels; the identity warp against od_augment_mosaic; the generator with the new options end to end."""
import pathlib
import sys

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

import warp_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (64, 48), (29, 31), (50, 50)]   # sources, (h, w)
OUTS = [(48, 64), (33, 47), (50, 50)]              # outputs: 48 x 64 has one wavefront per row, the others straddle rows
B = 3


def _sources(seed=12):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in SIZES]


def _tile(rng, plain=False):
    from object_detector_amd import od_gen
    p = od_gen.AugParams()
    if not plain:
        x1, y1 = rng.uniform(0, 0.3, 2)
        x2, y2 = rng.uniform(0.6, 1.0, 2)
        p.crop = (float(x1), float(y1), float(x2), float(y2))
        p.flip = bool(rng.random() < 0.5)
        p.brightness, p.contrast, p.saturation = float(rng.uniform(-32, 32)), float(rng.uniform(0.6, 1.4)), float(rng.uniform(0.6, 1.4))
    return p


def _mosaic(rng, hw, split=None):
    """-> (four source indices, MosaicParams without an erase list)"""
    from object_detector_amd import od_gen
    H, W = hw
    if split is None:
        split = (int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1)))
    return tuple(int(v) for v in rng.integers(0, len(SIZES), 4)), od_gen.MosaicParams(split, [_tile(rng) for _ in range(4)])


def _erase(rng, n):
    out = []
    for _ in range(n):
        x1, y1 = rng.uniform(0, 0.6, 2)
        out.append(((float(x1), float(y1), float(x1 + rng.uniform(0.1, 0.4)), float(y1 + rng.uniform(0.1, 0.4))),
                    tuple(int(v) for v in rng.integers(0, 256, 3))))
    return out


def _colour(rng):
    """A colour matrix off the HSV family: a hue / saturation / value turn, perturbed, with an offset column."""
    from object_detector_amd import od_gen
    k = od_gen.hsv_matrix(rng.uniform(-0.1, 0.1), rng.uniform(0.3, 1.7), rng.uniform(0.6, 1.4)).astype(np.float64)
    k[:, :3] += rng.uniform(-0.05, 0.05, (3, 3))
    k[:, 3] = rng.uniform(-20, 20, 3)
    return k


def _general_cases(hw, seed):
    """B output images: random affine (rotation up to 45 degrees, zoom 0.5 .. 1.5, shear, translation), random colour
    matrices, one and two frames, every frame a mosaic, erase after the mix -> (per image the frames' source indices,
    list[WarpParams])."""
    from object_detector_amd import od_gen
    rng = np.random.default_rng(seed)
    quads, wps = [], []
    for i in range(B):
        n = 1 + (i + seed) % 2
        frames = [_mosaic(rng, hw) for _ in range(n)]
        inv = [od_gen.affine_inverse(od_gen.sample_affine(rng, hw, degrees=45, translate=0.2, scale=0.5, shear=10)) for _ in range(n)]
        r = np.float32(rng.beta(2.0, 2.0))
        quads.append([f[0] for f in frames])
        wps.append(od_gen.WarpParams([f[1] for f in frames], inv, [_colour(rng) for _ in range(n)],
                                     (r, np.float32(1.0) - r) if n == 2 else (1.0, 0.0),
                                     tuple(int(v) for v in rng.integers(0, 256, 3)), _erase(rng, i)))
    assert {len(w.frames) for w in wps} == {1, 2}
    return quads, wps


def _check(out, src, quads, wps, hw):
    for i, (q, wp) in enumerate(zip(quads, wps)):
        ref = warp_ref.from_params(wp, [[src[j] for j in four] for four in q], hw)
        assert out[i].shape == ref.shape
        assert (out[i] == ref).all(), (i, hw, len(wp.frames), int(np.abs(out[i].astype(int) - ref.astype(int)).max()),
                                       int((out[i] != ref).any(-1).sum()))


@pytest.mark.parametrize("hw", OUTS)
def test_identity_warp_is_od_augment_mosaic(cuda, hw):
    """Identity matrix, identity colour, one frame: byte for byte the output of od_augment_mosaic on the same parameters --
    split = (W, H), splits on a wavefront boundary (at 48 x 64 a wavefront is one row: any split_y with split_x = W), a
    split inside a wavefront, random ones; with the erase list."""
    from object_detector_amd import od_gen
    H, W = hw
    src = _sources()
    rng = np.random.default_rng(H)
    for splits in ([(W, H), (W, H // 2), (W // 2, H // 3)], [(1, 1), (W - 1, H), None], [None, None, None]):
        ms = [_mosaic(rng, hw, sp) for sp in splits]
        erase = [_erase(rng, k) for k in range(B)]
        images = [tuple(src[j] for j in four) for four, _mp in ms]
        want = od_gen.apply_mosaic_device(images, [od_gen.MosaicParams(mp.split, mp.tiles, e) for (_f, mp), e in zip(ms, erase)],
                                          hw, cuda)
        got = od_gen.apply_warp_device([[im] for im in images],
                                       [od_gen.WarpParams([mp], erase=e) for (_f, mp), e in zip(ms, erase)], hw, cuda)
        assert torch.equal(got, want), [mp.split for _f, mp in ms]


def test_quarter_turn_is_rot90(cuda):
    """50 x 50 source, full crop, no colour change, to a 50 x 50 output through the inverse matrix fx = py, fy = 50 - px:
    output pixel (x, y) shows source pixel (column y, row 49 - x) -- the picture is turned by 90 degrees CLOCKWISE as it is
    displayed (y down), which is np.rot90(src, -1)."""
    from object_detector_amd import od_gen
    src = _sources()[3]
    mp = od_gen.MosaicParams.single(od_gen.AugParams(), (50, 50))
    wp = od_gen.WarpParams([mp], inv=[(0, 1, 0, -1, 0, 50)])
    out = od_gen.apply_warp_device([[(src, None, None, None)]], [wp], (50, 50), cuda).cpu().numpy()[0]
    assert (out == np.rot90(src, -1)).all()
    assert (out == warp_ref.from_params(wp, [(src, None, None, None)], (50, 50))).all()


@pytest.mark.parametrize("hw", OUTS)
def test_general_case_bit_exact_packed_host_route(cuda, hw):
    from object_detector_amd import od_gen
    src = _sources()
    quads, wps = _general_cases(hw, seed=hw[0])
    out = od_gen.apply_warp_device([[tuple(src[j] for j in four) for four in q] for q in quads], wps, hw, cuda).cpu().numpy()
    _check(out, src, quads, wps, hw)


@pytest.mark.parametrize("hw", OUTS)
def test_general_case_bit_exact_resident_route_with_negative_offsets(cuda, hw):
    """Every source a device tensor of its own allocation; the base pointer (the first source handed over) is the HIGHEST
    address, so every other offset is negative."""
    from object_detector_amd import od_gen
    src = _sources()
    dev = [torch.from_numpy(a).to(cuda) for a in src]
    assert len({t.data_ptr() for t in dev}) == len(dev)
    quads, wps = _general_cases(hw, seed=hw[0] + 1)
    order = np.argsort([t.data_ptr() for t in dev])
    quads[0][0] = (int(order[-1]), int(order[0]), int(order[1]), int(order[2]))
    wps[0].frames[0].split = (hw[1] // 2, hw[0] // 2)
    base = dev[quads[0][0][0]].data_ptr()
    assert all(dev[j].data_ptr() - base <= 0 for q in quads for four in q for j in four)
    assert any(dev[j].data_ptr() - base < 0 for q in quads for four in q for j in four)
    out = od_gen.apply_warp_device([[tuple(dev[j] for j in four) for four in q] for q in quads], wps, hw, cuda).cpu().numpy()
    _check(out, src, quads, wps, hw)


def test_outside_mix_weights_and_guard_bands(cuda):
    from object_detector_amd import od_gen
    hw = (33, 47)
    H, W = hw
    src = _sources()
    quads, wps = _general_cases(hw, seed=9)
    images = [[tuple(src[j] for j in four) for four in q] for q in quads]
    # a translation that puts the whole frame outside: fill_rgb everywhere (the erase list still acts: none here)
    gone = [od_gen.WarpParams(wp.frames, [(1, 0, 2 * W, 0, 1, 0)] * len(wp.frames), wp.colour, wp.mix, (7 + i, 114, 250 - i))
            for i, wp in enumerate(wps)]
    out = od_gen.apply_warp_device(images, gone, hw, cuda).cpu().numpy()
    for i in range(B):
        assert (out[i] == np.array([7 + i, 114, 250 - i], np.uint8)).all()
    # mix_a = 1, mix_b = 0: frame A alone
    two = [i for i, wp in enumerate(wps) if len(wp.frames) == 2]
    assert two
    a_only = [od_gen.WarpParams(wp.frames, wp.inv, wp.colour, (1.0, 0.0), wp.fill, wp.erase) for wp in wps]
    alone = [od_gen.WarpParams(wp.frames[:1], wp.inv[:1], wp.colour[:1], (1.0, 0.0), wp.fill, wp.erase) for wp in wps]
    got = od_gen.apply_warp_device(images, a_only, hw, cuda)
    want = od_gen.apply_warp_device([q[:1] for q in images], alone, hw, cuda)
    assert torch.equal(got, want)
    _check(got.cpu().numpy(), src, quads, a_only, hw)
    # guard bands before and after the output stay as they were
    n, guard = B * H * W * 3, 4096
    buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=cuda)
    view = buf[guard:guard + n].view(B, H, W, 3)
    res = od_gen.apply_warp_device(images, wps, hw, cuda, out=view)
    assert res.data_ptr() == view.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + n:] == 0xA5).all()
    _check(host[guard:guard + n].reshape(B, H, W, 3), src, quads, wps, hw)


def test_argument_checks(cuda, monkeypatch):
    """Host-side ValueErrors fire before any launch; the C entry refuses null pointers and sizes out of range."""
    from object_detector_amd import _lib, od_gen
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    launches = []
    real = ctx.lib.od_augment_warp
    img = np.zeros((8, 8, 3), np.uint8)
    dimg = torch.zeros((8, 8, 3), dtype=torch.uint8, device=cuda)
    tiles = [od_gen.AugParams() for _ in range(4)]
    ok = od_gen.MosaicParams((4, 4), tiles)
    quad = (img,) * 4

    class _Lib:  # counts what reaches the entry
        def __getattr__(self, name):
            if name == "od_augment_warp":
                return lambda *a: launches.append(a) or real(*a)
            return getattr(ctx.lib, name)
    with monkeypatch.context() as m:
        m.setattr(ctx, "lib", _Lib())
        with pytest.raises(ValueError, match="n_frames"):
            od_gen.apply_warp_device([[quad] * 3], [od_gen.WarpParams([ok] * 3)], (8, 8), cuda)
        with pytest.raises(ValueError, match="n_frames"):
            od_gen.apply_warp_device([[]], [od_gen.WarpParams([])], (8, 8), cuda)
        with pytest.raises(ValueError, match="n_frames"):
            od_gen.apply_warp_device([[quad]], [od_gen.WarpParams([ok, ok])], (8, 8), cuda)  # two frames, one source quad
        for split in ((0, 4), (4, 9), (9, 4)):
            with pytest.raises(ValueError, match="split"):
                od_gen.apply_warp_device([[quad]], [od_gen.WarpParams([od_gen.MosaicParams(split, tiles)])], (8, 8), cuda)
        with pytest.raises(ValueError, match="no source"):
            od_gen.apply_warp_device([[(img, None, img, img)]], [od_gen.WarpParams([ok])], (8, 8), cuda)
        with pytest.raises(ValueError, match="erase"):
            od_gen.apply_warp_device([[quad]], [od_gen.WarpParams([od_gen.MosaicParams((4, 4), tiles, [((0, 0, 1, 1), (1, 1, 1))])])],
                                     (8, 8), cuda)
        bad = [od_gen.AugParams() for _ in range(4)]
        bad[0].erase = [((0, 0, 1, 1), (1, 1, 1))]
        with pytest.raises(ValueError, match="erase"):
            od_gen.apply_warp_device([[quad]], [od_gen.WarpParams([od_gen.MosaicParams((4, 4), bad)])], (8, 8), cuda)
        with pytest.raises(ValueError, match="all host arrays or all device tensors"):
            od_gen.apply_warp_device([[(img, dimg, img, img)]], [od_gen.WarpParams([ok])], (8, 8), cuda)
        assert launches == []
        od_gen.apply_warp_device([[quad]], [od_gen.WarpParams([ok])], (8, 8), cuda)
        assert len(launches) == 1
    # the C entry
    prm = torch.zeros(_lib.load().od_warp_params_bytes(), dtype=torch.uint8, device=cuda)
    out = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=cuda)
    h, s, p, o = ctx.handle, dimg.data_ptr(), prm.data_ptr(), out.data_ptr()
    for args in ((None, s, p, o, 1, 8, 8), (h, None, p, o, 1, 8, 8), (h, s, None, o, 1, 8, 8), (h, s, p, None, 1, 8, 8),
                 (h, s, p, o, 0, 8, 8), (h, s, p, o, 65536, 8, 8), (h, s, p, o, 1, 0, 8), (h, s, p, o, 1, 8, -1)):
        assert real(*args, None) != 0, args
        assert b"od_augment_warp" in ctx.lib.od_last_error()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0  # none of them launched


def test_generator_with_warp_hsv_mixup_end_to_end(cuda):
    """160 x 160, B = 8, mosaic + affine + hsv + mixup on the resident route: shapes, dtypes and counters are consistent with
    the annotations, every box lies inside [0, 1] and is at least min_px wide, and batch 0 re-rendered through warp_ref from
    the recorded parameters gives the same bytes."""
    import _common
    from object_detector_amd import od_gen
    X, y = _common.shapes_dataset(24, seed=5, difficult_frac=0.2, crowd_frac=0.4)
    S, Bg, n = 160, 8, 4

    def run(prefetch=0):
        gen = od_gen.create_generator((S, S), device=cuda, on_device=True, device_cache=True, mosaic=0.5, ignore_regions=True,
                                      affine={"degrees": 10, "translate": 0.1, "scale": 0.5, "shear": 2}, hsv=(0.015, 0.7, 0.4),
                                      mixup=0.3)
        g, _ = gen.flow(X, y, batch_size=Bg, data_augmentation=True, shuffle=True, seed=21, prefetch=prefetch)
        out, recs = [], []
        for _ in range(n):
            xb, anns = next(g)
            torch.cuda.synchronize()
            assert xb.is_cuda and xb.dtype == torch.uint8 and tuple(xb.shape) == (Bg, S, S, 3) and len(anns) == Bg
            out.append((xb.cpu().numpy().copy(), anns))
            recs.append(gen.last_warp)
        g.close()
        return out, recs, dict(gen.stats)
    a, recs, st = run()
    assert st["warps"] == n * Bg and 0 < st["mixups"] < n * Bg and 0 < st["mosaics"]
    wps = [wp for r in recs for _fours, wp in r]
    assert sum(len(wp.frames) == 2 for wp in wps) == st["mixups"]
    assert sum(mp.split != (S, S) for wp in wps for mp in wp.frames) == st["mosaics"]
    for _xb, anns in a:
        for an in anns:
            assert an.bboxes.dtype == np.float32 and len(an.classes) == len(an.bboxes) == len(an.difficults) <= 128
            assert (an.bboxes >= 0).all() and (an.bboxes <= 1).all()
            assert ((an.bboxes[:, 2:] - an.bboxes[:, :2]) * S >= 2.0 - 1e-4).all()  # min_px = 2 output pixels, f32 boxes
    assert sum(an.num_objects for _x, anns in a for an in anns) > 0
    for k, (fours, wp) in enumerate(recs[0]):
        images = [tuple(np.asarray(X[j])[..., :3] if j is not None else None for j in four) for four in fours]
        ref = warp_ref.from_params(wp, images, (S, S))
        assert (a[0][0][k] == ref).all(), (k, len(wp.frames), int((a[0][0][k] != ref).any(-1).sum()))
    # the same seed gives the same stream, from the prefetch thread too
    b, _r, sb = run(prefetch=2)  # its counters run ahead of the batches consumed: at least as many
    assert sb["warps"] >= st["warps"] and sb["warps"] % Bg == 0
    for (xa, ya), (xb, yb) in zip(a, b):
        assert xa.tobytes() == xb.tobytes()
        assert all(np.array_equal(p.bboxes, q.bboxes) and np.array_equal(p.difficults, q.difficults) for p, q in zip(ya, yb))


def test_check_generator_script_with_the_new_options(cuda, tmp_path):
    """scripts/check_generator.py --affine --hsv --mixup (with and without --mosaic), each a fresh child process."""
    import subprocess
    warp = ["--affine", "10", "0.1", "0.5", "2", "--hsv", "0.015", "0.7", "0.4", "--mixup", "0.5"]
    for name, extra in (("warp", warp), ("warp_mosaic", warp + ["--mosaic", "0.5"])):
        out = tmp_path / name
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / "check_generator.py"), "--synthetic", "1", "--batches", "2",
                            "--save-dir", str(out)] + extra, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(list(out.glob("[0-9].jpg"))) == 2  # one picture per batch
