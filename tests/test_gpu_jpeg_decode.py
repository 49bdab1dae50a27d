"""image_decode="device" (csrc/jpeg.hip, devdecode.py): the device-written network input equals imageio.load_image byte
for byte, predictions equal the host route's, and corrupt entropy data stays inside its buffers."""
import io
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

from object_detector_amd import devdecode
from object_detector_amd.imageio import load_image

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 3), (15, 9), (17, 33), (500, 375), (375, 500), (1023, 769)]  # (w, h)
SAMPLING = [0, 1, 2, "L"]  # 4:4:4, 4:2:2, 4:2:0, grey


def _image(w, h, seed):
    """Smooth content plus noise: JPEG-typical coefficients, with detail at every scale."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (max(2, h // 16), max(2, w // 16), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR), np.int32)
    return np.clip(a + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)


def _jpeg(path, a, samp, **kw):
    img = Image.fromarray(a)
    if samp == "L":
        img.convert("L").save(path, "JPEG", **kw)
    else:
        img.save(path, "JPEG", subsampling=samp, **kw)
    return str(path)


def _decode(items, size, device):
    dec = devdecode.BatchDecoder(device)
    out = torch.zeros((len(items),) + tuple(size) + (3,), dtype=torch.uint8, device=device)
    dec.run(items, out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dec


@pytest.fixture(scope="module")
def matrix(tmp_path_factory):
    """Every size x sampling; quality, optimize and restart markers rotate over the four files of each pair."""
    d = tmp_path_factory.mktemp("jpg")
    opts = [dict(quality=10, optimize=True), dict(quality=75, optimize=True), dict(quality=95, restart_marker_blocks=2),
            dict(quality=100, restart_marker_rows=1)]  # PIL cannot write optimize=True at 4:4:4 quality 100
    paths = []
    for n, ((w, h), samp) in enumerate(itertools.product(SIZES, SAMPLING)):
        a = _image(w, h, n)
        for k, kw in enumerate(opts):
            kw = dict(opts[(k + n) % 4])
            paths.append(_jpeg(d / f"{n}_{k}.jpg", a, samp, **kw))
    return paths


@pytest.mark.parametrize("size,keep_aspect", [((320, 320), False), ((320, 320), True), ((640, 640), False),
                                              ((640, 640), True)])
def test_device_input_equals_host_input(cuda, matrix, size, keep_aspect):
    items = [devdecode.prepare(p, size, keep_aspect) for p in matrix]
    assert all(it[0] == "jpeg" for it in items)
    got, dec = _decode(items, size, cuda)
    assert min(dec.sync_rounds()) >= 1
    for i, p in enumerate(matrix):
        ref, sc = load_image(p, size, keep_aspect, True)
        assert items[i][3] == sc
        if not np.array_equal(got[i], ref):
            diff = np.argwhere(got[i] != ref)
            pytest.fail(f"{p} ({Image.open(p).size}, {Image.open(p).layer}): {len(diff)} bytes differ, first {diff[:4].tolist()}")


def _fallback_files(d):
    a = _image(61, 47, 7)
    out = {}
    for name, kw in (("progressive", dict(progressive=True)), ("default", {})):
        out[name] = _jpeg(d / f"{name}.jpg", a, 2, **kw)
    Image.fromarray(a).save(d / "p.png")
    out["png"] = str(d / "p.png")
    Image.fromarray(a).convert("CMYK").save(d / "cmyk.jpg", "JPEG")
    out["cmyk"] = str(d / "cmyk.jpg")
    return out  # a file without EOI also falls back (tests/test_jpeg_host.py), but PIL refuses it on either route


def test_fallback_routes_and_stats(cuda, tmp_path):
    from object_detector_amd.detector import ObjectDetector
    files = _fallback_files(tmp_path)
    size = (96, 96)
    for keep_aspect in (False, True):
        X = [files[k] for k in ("progressive", "png", "cmyk", "default")]
        X += [_image(40, 30, 3), _image(96, 96, 4), _image(50, 70, 5).astype(np.float32) * 1.5,
              np.dstack([_image(33, 20, 6), np.full((20, 33, 1), 9, np.uint8)])]
        items = [devdecode.prepare(x, size, keep_aspect) for x in X]
        assert [it[0] for it in items] == ["fallback"] * 3 + ["jpeg"] + ["array"] * 4
        got, _ = _decode(items, size, cuda)
        for i, x in enumerate(X):
            ref, sc = load_image(x, size, keep_aspect, True)
            assert items[i][3] == sc
            np.testing.assert_array_equal(got[i], ref, err_msg=f"input {i}")
    od = ObjectDetector.synthetic(4, size, seed=2, device=cuda, use_multi_gpu=False, image_decode="device")
    od.predict(X, conf_threshold=0.3)
    assert od.decode_stats == {"jpeg": 1, "fallback": 3, "array": 4}


@pytest.mark.parametrize("keep_aspect", [False, True])
def test_predictions_identical(cuda, tmp_path, keep_aspect):
    from object_detector_amd.detector import ObjectDetector
    X = []
    for i in range(75):  # 32 + 32 + 11: a ragged last batch
        w, h = (500, 375) if i % 3 else (160 + 7 * i, 120 + 3 * i)
        a = _image(w, h, 100 + i)
        if i % 5 == 4:
            X.append(a)
        elif i % 7 == 6:
            Image.fromarray(a).save(tmp_path / f"{i}.png")
            X.append(str(tmp_path / f"{i}.png"))
        else:
            X.append(_jpeg(tmp_path / f"{i}.jpg", a, i % 3, quality=70 + i % 30))
    od = ObjectDetector.synthetic(32, (320, 320), seed=2, device=cuda, use_multi_gpu=False, keep_aspect=keep_aspect,
                                  image_decode="device")
    dev = od.predict(X, conf_threshold=0.05)
    host = od.predict(X, conf_threshold=0.05, image_decode="host")
    assert od.decode_stats["jpeg"] > 40 and od.decode_stats["array"] == 15
    assert sum(len(p) for p in host) > 0
    for i, (a, b) in enumerate(zip(dev, host)):
        assert np.array_equal(a.classes, b.classes), i
        assert np.array_equal(a.confs, b.confs), i
        assert np.array_equal(a.bboxes, b.bboxes), i


def test_corrupt_streams_stay_in_bounds(cuda, tmp_path):
    """Random bit flips in the entropy-coded data: no error, nothing written outside the batch's buffers, and the next
    clean batch is exact."""
    size = (320, 320)
    rng = np.random.default_rng(5)
    clean, bad = [], []
    for i in range(12):
        a = _image(200 + 13 * i, 150 + 7 * i, 300 + i)
        p = _jpeg(tmp_path / f"c{i}.jpg", a, i % 4 if i % 4 < 3 else "L", quality=90,
                  **({"restart_marker_blocks": 3} if i % 2 else {}))
        clean.append(p)
        data = bytearray(open(p, "rb").read())
        sos = data.index(b"\xff\xda")
        lo = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
        for pos in rng.integers(lo, len(data) - 2, 24):
            data[pos] ^= 1 << int(rng.integers(0, 8))
        q = tmp_path / f"b{i}.jpg"
        q.write_bytes(bytes(data))
        bad.append(str(q))
    items = []
    for p in bad:
        try:
            it = devdecode.prepare(p, size, False)
        except OSError:  # a flip made a marker: PIL's fallback refuses the file, as the host route would
            continue
        if it[0] == "jpeg":
            items.append(it)
    assert len(items) >= 6
    dec = devdecode.BatchDecoder(cuda)
    guard = 0xA5
    dec.pinned = torch.full((8 << 20,), guard, dtype=torch.uint8).pin_memory()
    dec.blob = torch.full((8 << 20,), guard, dtype=torch.uint8, device=cuda)
    dec.ws = torch.full((64 << 20,), guard, dtype=torch.uint8, device=cuda)
    out = torch.full((len(items) + 2,) + size + (3,), guard, dtype=torch.uint8, device=cuda)
    dec.run(items, out[1:-1])
    torch.cuda.synchronize()
    blob_used, ws_used = dec.used
    assert blob_used < dec.blob.numel() and ws_used < dec.ws.numel()
    assert bool((dec.blob[blob_used:] == guard).all())
    assert bool((dec.ws[ws_used:] == guard).all())
    assert bool((out[0] == guard).all()) and bool((out[-1] == guard).all())
    items = [devdecode.prepare(p, size, False) for p in clean]
    out2 = torch.zeros((len(items),) + size + (3,), dtype=torch.uint8, device=cuda)
    dec.run(items, out2)
    got = out2.cpu().numpy()
    for i, p in enumerate(clean):
        np.testing.assert_array_equal(got[i], load_image(p, size), err_msg=p)
