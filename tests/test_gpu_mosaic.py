"""GPU parity of od_augment_mosaic (K14, four sources per output image) against tests/mosaic_ref.py, byte for byte; the
degenerate mosaic against od_augment_batch; the generator with mosaic end to end."""
import pathlib
import sys

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))

import mosaic_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(375, 500), (97, 61), (33, 47), (1, 1), (240, 401), (512, 512), (7, 300)]


def _tile(rng, k):
    from object_detector_amd import od_gen
    p = od_gen.AugParams()
    if k % 4 != 3:
        x1, y1 = rng.uniform(0, 0.3, 2)
        x2, y2 = rng.uniform(0.6, 1.0, 2)
        p.crop = (float(x1), float(y1), float(x2), float(y2))
        p.flip = bool(k % 2)
        p.brightness, p.contrast, p.saturation = float(rng.uniform(-32, 32)), float(rng.uniform(0.6, 1.4)), float(rng.uniform(0.6, 1.4))
    return p


def _cases(H, W, seed):
    """-> images (list of 4-tuples of indices into the source list), list[MosaicParams]: fixed corner splits + random ones."""
    from object_detector_amd import od_gen
    rng = np.random.default_rng(seed)
    splits = [(W, H), (W, H // 3), (W // 2, H), (1, 1), (1, H), (W, 1), (W - 1, H - 1), (1, H // 2), (W // 2, H // 2)]
    splits += [(int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))) for _ in range(7)]
    quads, mps = [], []
    for k, sp in enumerate(splits):
        quads.append(tuple(int(v) for v in rng.integers(0, len(SIZES), 4)))
        if k == 3:
            quads[-1] = (3, 0, 1, 2)  # the 1x1 source in a one-pixel tile
        if k == 4:
            quads[-1] = (0, 3, 3, 1)  # ... and stretched over big tiles
        erase = []
        if k % 2 == 0:  # rectangles across the split lines, overlapping one another
            cx, cy = sp[0] / W, sp[1] / H
            erase = [((max(0.0, cx - 0.2), max(0.0, cy - 0.1), min(1.0, cx + 0.15), min(1.0, cy + 0.2)), (1, 2, 3)),
                     ((0.05, max(0.0, cy - 0.05), 0.95, min(1.0, cy + 0.05)), (250, 128, 7)),
                     ((max(0.0, cx - 0.03), 0.0, min(1.0, cx + 0.04), 1.0), (0, 255, 99))][:1 + k % 3]
        mps.append(od_gen.MosaicParams(sp, [_tile(rng, k + t) for t in range(4)], erase))
    return quads, mps


def _sources(seed=12):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


def _check(out, src, quads, mps, hw):
    for i, (q, mp) in enumerate(zip(quads, mps)):
        ref = mosaic_ref.mosaic([src[j] for j in q], hw, mp.split, mp.tiles, mp.erase)
        assert out[i].shape == ref.shape
        assert (out[i] == ref).all(), (i, mp.split, int(np.abs(out[i].astype(int) - ref.astype(int)).max()),
                                      int((out[i] != ref).any(-1).sum()))


@pytest.mark.parametrize("hw", [(320, 320), (640, 640), (128, 160)])
def test_mosaic_bit_exact_packed_host_route(cuda, hw):
    from object_detector_amd import od_gen
    src = _sources()
    quads, mps = _cases(hw[0], hw[1], seed=hw[0])
    out = od_gen.apply_mosaic_device([tuple(src[j] for j in q) for q in quads], mps, hw, cuda).cpu().numpy()
    _check(out, src, quads, mps, hw)


@pytest.mark.parametrize("hw", [(320, 320), (640, 640)])
def test_mosaic_bit_exact_resident_route_with_negative_offsets(cuda, hw):
    """Every source a device tensor of its own allocation, handed over in an order that is not the address order: the tile
    offsets are signed."""
    from object_detector_amd import od_gen
    src = _sources()
    dev = [torch.from_numpy(a).to(cuda) for a in src]
    quads, mps = _cases(hw[0], hw[1], seed=hw[0] + 1)
    order = np.argsort([t.data_ptr() for t in dev])
    assert len({t.data_ptr() for t in dev}) == len(dev)
    quads[0] = (int(order[-1]), int(order[0]), int(order[1]), int(order[2]))  # the base is the HIGHEST address
    mps[0].split = (hw[1] // 2, hw[0] // 2)
    base = dev[quads[0][0]].data_ptr()
    assert any(dev[j].data_ptr() - base < 0 for q in quads for j in q)
    out = od_gen.apply_mosaic_device([tuple(dev[j] for j in q) for q in quads], mps, hw, cuda).cpu().numpy()
    _check(out, src, quads, mps, hw)


def test_degenerate_mosaic_equals_augment_batch(cuda):
    """split = (W, H): the TL tile is the frame; byte-identical to od_augment_batch for the parameter sets of
    tests/test_gpu_train_ops.py::test_augment_batch_bit_exact, erase rectangles included."""
    from object_detector_amd import od_gen
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(375, 500), (96, 64), (33, 47), (512, 512)]]
    prm = []
    for i in range(4):
        p = od_gen.AugParams()
        if i != 3:
            p.crop = (0.05 * i, 0.1, 0.9, 1.0 - 0.07 * i)
            p.flip = bool(i % 2)
            p.brightness, p.contrast, p.saturation = 10.0 * i - 12, 0.8 + 0.2 * i, 1.3 - 0.25 * i
            p.erase = [((0.1, 0.2, 0.4, 0.5), (1, 2, 3)), ((0.5, 0.5, 0.95, 0.9), (200, 100, 50))][:i + 1]
        prm.append(p)
    for hw in ((128, 160), (320, 320)):
        a = od_gen.apply_pixels_device(imgs, prm, hw, cuda)
        mps = [od_gen.MosaicParams.single(p, hw) for p in prm]
        b = od_gen.apply_mosaic_device([(im, None, None, None) for im in imgs], mps, hw, cuda)
        assert torch.equal(a, b)
        dev = [torch.from_numpy(im).to(cuda) for im in imgs]
        c = od_gen.apply_mosaic_device([(im, None, None, None) for im in dev], mps, hw, cuda)
        assert torch.equal(a, c)


def test_mosaic_argument_checks(cuda):
    from object_detector_amd import od_gen
    img = np.zeros((8, 8, 3), np.uint8)
    tiles = [od_gen.AugParams() for _ in range(4)]
    with pytest.raises(ValueError, match="split"):
        od_gen.apply_mosaic_device([(img,) * 4], [od_gen.MosaicParams((0, 4), tiles)], (8, 8), cuda)
    with pytest.raises(ValueError, match="no source"):
        od_gen.apply_mosaic_device([(img, None, img, img)], [od_gen.MosaicParams((4, 4), tiles)], (8, 8), cuda)
    tiles[0].erase = [((0, 0, 1, 1), (1, 1, 1))]
    with pytest.raises(ValueError, match="erase"):
        od_gen.apply_mosaic_device([(img,) * 4], [od_gen.MosaicParams((4, 4), tiles)], (8, 8), cuda)


def _run(cuda, X, y, n_batches, B=8, S=160, **kw):
    from object_detector_amd import od_gen
    from object_detector_amd.pb import PriorBoxes
    prefetch = kw.pop("prefetch", 0)
    pb = PriorBoxes((S, S), 20, device=cuda, ignore_regions=kw.get("ignore_regions", False))
    gen = od_gen.create_generator((S, S), encode_truth=pb.encode_truth_device, device=cuda, on_device=True, device_cache=True, **kw)
    g, _ = gen.flow(X, y, batch_size=B, data_augmentation=True, shuffle=True, seed=21, prefetch=prefetch)
    out = []
    for _ in range(n_batches):
        xb, yb = next(g)
        torch.cuda.synchronize()
        out.append((xb.cpu().numpy().copy(), yb.cpu().numpy().copy()))
    stats = dict(gen.stats)
    g.close()
    return out, stats


def test_generator_with_mosaic_end_to_end(cuda):
    import _common
    X, y = _common.shapes_dataset(24, seed=5, difficult_frac=0.2, crowd_frac=0.4)
    n, B = 7, 8  # more than two epochs of 3 batches: first decoded, then resident
    a, sa = _run(cuda, X, y, n, B, mosaic=1.0, ignore_regions=True)
    b, sb = _run(cuda, X, y, n, B, mosaic=1.0, ignore_regions=True)
    c, _sc = _run(cuda, X, y, n, B, mosaic=1.0, ignore_regions=True, prefetch=2)
    for (xa, ya), (xb, yb), (xc, yc) in zip(a, b, c):
        assert xa.tobytes() == xb.tobytes() and ya.tobytes() == yb.tobytes()   # the same seed, twice
        assert xa.tobytes() == xc.tobytes() and ya.tobytes() == yc.tobytes()   # ... and from the prefetch thread
        assert np.isfinite(ya).all() and xa.shape == (B, 160, 160, 3)
    assert sa == sb and sa["mosaics"] == n * B
    assert sa["boxes_ignored"] > 0  # slivers at tile borders became ignore regions (drops are rarer: not demanded here)
    assert any((ya[..., 1] == 1).any() for _x, ya in a)
    # a mosaic is not the plain image
    plain, sp = _run(cuda, X, y, 2, B)
    assert sp["mosaics"] == 0 and plain[0][0].tobytes() != a[0][0].tobytes()
    # mosaic = 0.0: byte-identical to a generator built without the argument
    off, so = _run(cuda, X, y, 2, B, mosaic=0.0)
    for (xa, ya), (xb, yb) in zip(plain, off):
        assert xa.tobytes() == xb.tobytes() and ya.tobytes() == yb.tobytes()
    assert so["mosaics"] == 0
    # a mixed stream (some images mosaics, some riding along as degenerate ones) is reproducible too
    m1, s1 = _run(cuda, X, y, 4, B, mosaic=0.5)
    m2, s2 = _run(cuda, X, y, 4, B, mosaic=0.5)
    assert s1 == s2 and 0 < s1["mosaics"] < 4 * B and s1["boxes_ignored"] == 0
    for (xa, ya), (xb, yb) in zip(m1, m2):
        assert xa.tobytes() == xb.tobytes() and ya.tobytes() == yb.tobytes()


def test_generator_mosaic_host_batches_and_no_device_cache(cuda):
    """on_device=False / device_cache=False (the packed-host route, numpy batches, annotations out): same images as the
    resident route."""
    import _common
    from object_detector_amd import od_gen
    X, y = _common.shapes_dataset(12, seed=6)
    outs = []
    for kw in ({"on_device": True, "device_cache": True}, {}):
        gen = od_gen.create_generator((96, 128), device=cuda, mosaic=1.0, **kw)
        g, _ = gen.flow(X, y, batch_size=4, data_augmentation=True, shuffle=True, seed=2)
        outs.append([next(g) for _ in range(4)])
    for (xa, ya), (xb, yb) in zip(*outs):
        assert isinstance(xb, np.ndarray) and np.array_equal(xa.cpu().numpy(), xb)
        for p, q in zip(ya, yb):
            assert np.array_equal(p.bboxes, q.bboxes) and np.array_equal(p.difficults, q.difficults)
            assert (p.bboxes >= 0).all() and (p.bboxes <= 1).all()


def test_checker_scripts_with_the_new_options(cuda, tmp_path):
    """scripts/check_generator.py --mosaic P and scripts/check_assign.py --ignore-regions, each a fresh child process."""
    import subprocess
    for script, extra in (("check_generator.py", ["--mosaic", "0.5"]), ("check_assign.py", ["--ignore-regions"])):
        out = tmp_path / script[:-3]
        r = subprocess.run([sys.executable, str(ROOT / "scripts" / script), "--synthetic", "1", "--batches", "2", "--save-dir",
                            str(out)] + extra, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(list(out.glob("[0-9].jpg"))) == 2  # one picture per batch
        if script == "check_assign.py":
            assert len(list(out.glob("*_ignored.jpg"))) == 2
