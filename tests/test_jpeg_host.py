"""Host side of image_decode="device" (no GPU): Pillow-exact BILINEAR tables (resample.py), the JPEG header parser
(jpeg.py), and a numpy reference of the device decoder's stages (jpeg_ref.py) against PIL's decode."""
import io
import itertools
import pathlib
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import jpeg_ref  # noqa: E402

from object_detector_amd import jpeg, resample  # noqa: E402
from object_detector_amd.imageio import load_image  # noqa: E402


def _image(w, h, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (max(2, h // 8), max(2, w // 8), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR), np.int32)
    return np.clip(a + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)


def _encode(a, samp=2, grey=False, **kw):
    f = io.BytesIO()
    img = Image.fromarray(a)
    if grey:
        img.convert("L").save(f, "JPEG", **kw)
    else:
        img.save(f, "JPEG", subsampling=samp, **kw)
    return f.getvalue()


@pytest.mark.parametrize("src_wh,dst_wh", [
    ((500, 375), (320, 320)), ((375, 500), (320, 320)), ((77, 100), (320, 320)), ((1920, 1080), (320, 320)),
    ((320, 320), (320, 320)), ((1, 1), (320, 320)), ((1, 9), (5, 1)), ((640, 480), (416, 416)), ((7, 300), (320, 320)),
    ((500, 375), (320, 240)), ((500, 375), (640, 480)), ((375, 500), (240, 320)), ((1920, 1080), (640, 360)),
])
def test_resample_equals_pil(src_wh, dst_wh):
    a = _image(*src_wh, seed=sum(src_wh))
    ref = np.asarray(Image.fromarray(a).resize(dst_wh, Image.BILINEAR))
    np.testing.assert_array_equal(resample.resize(a, dst_wh), ref)


@pytest.mark.parametrize("size", [(320, 320), (640, 640)])
def test_letterbox_matches_load_image(size):
    for wh in ((500, 375), (375, 500), (1, 1), (1023, 769)):
        a = _image(*wh, seed=3)
        ref, sc = load_image(a, size, keep_aspect=True, return_scale=True)
        (nw, nh), sc2 = resample.letterbox_size(a.shape[:2], size, True)
        assert sc == sc2
        canvas = np.zeros(size + (3,), np.uint8)
        canvas[:nh, :nw] = resample.resize(a, (nw, nh))
        np.testing.assert_array_equal(canvas, ref)


@pytest.mark.parametrize("samp,grey", [(0, False), (1, False), (2, False), (2, True)])
def test_parser_matches_pil(samp, grey):
    data = _encode(_image(53, 37, 1), samp, grey, quality=83)
    info = jpeg.parse(data)
    im = Image.open(io.BytesIO(data))
    assert (info.width, info.height) == im.size
    assert info.ncomp == len(im.layer)
    assert [(h, v) for _, h, v, _ in im.layer][:1] == info.samp[:1] or grey
    for ci, (_, _, _, tq) in enumerate(im.layer):
        np.testing.assert_array_equal(info.quant[ci], np.asarray(im.quantization[tq]))  # both natural order
    s = info.stream
    assert not np.any((s[:-1] == 0xFF) & (s[1:] == 0x00))
    assert info.n_blocks == info.mcux * info.mcuy * info.bpm


def test_unstuffing_removes_every_stuffed_zero():
    data = _encode(_image(64, 64, 2), 0, quality=100)
    raw = data[data.index(b"\xff\xda"):]
    assert raw.count(b"\xff\x00") > 0
    info = jpeg.parse(data)
    assert len(info.stream) < len(raw)
    assert not np.any((info.stream[:-1] == 0xFF) & (info.stream[1:] == 0x00))


@pytest.mark.parametrize("kw,mcus", [(dict(restart_marker_blocks=1), None), (dict(restart_marker_blocks=5), None),
                                     (dict(restart_marker_rows=1), "row"), (dict(restart_marker_rows=2), "row2")])
def test_restart_intervals(kw, mcus):
    data = _encode(_image(77, 45, 3), 2, quality=80, **kw)
    info = jpeg.parse(data)
    total = info.mcux * info.mcuy
    if mcus == "row":
        assert info.restart == info.mcux
    elif mcus == "row2":
        assert info.restart == 2 * info.mcux
    assert info.n_seg == -(-total // info.restart)
    sos = data.index(b"\xff\xda")
    n_rst = sum(data[sos:].count(bytes([0xFF, 0xD0 + k])) for k in range(8))
    assert n_rst == info.n_seg - 1
    subs = info.subsequences()
    assert subs[:, 5].sum() == info.n_seg and subs[-1, 4] == info.n_blocks
    assert np.all(subs[:, 1] <= subs[:, 2]) and np.all(subs[:, 0] < subs[:, 1])


def test_fallback_kinds(tmp_path):
    a = _image(40, 30, 4)
    prog = _encode(a, 2, progressive=True)
    f = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(f, "JPEG")
    cmyk = f.getvalue()
    f = io.BytesIO()
    Image.fromarray(a).save(f, "PNG")
    png = f.getvalue()
    good = _encode(a, 2)
    for data in (prog, cmyk, png, good[:-2], good[:len(good) // 2], good[:100]):
        with pytest.raises(jpeg.Fallback):
            jpeg.parse(data)
    jpeg.parse(good)


SMALL = [(1, 1), (3, 3), (9, 15), (16, 16), (17, 33), (48, 48), (5, 2), (2, 5), (47, 31)]


@pytest.mark.parametrize("samp,grey", [(0, False), (1, False), (2, False), (2, True)])
@pytest.mark.parametrize("kw", [dict(quality=10), dict(quality=75), dict(quality=100), dict(quality=90, optimize=True),
                                dict(quality=75, restart_marker_blocks=2)])
def test_reference_decoder_equals_pil(samp, grey, kw):
    for k, (w, h) in enumerate(SMALL):
        data = _encode(_image(w, h, 10 + k), samp, grey, **kw)
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        got = jpeg_ref.decode(jpeg.parse(data))
        np.testing.assert_array_equal(got, ref, err_msg=f"{w}x{h}")


def test_reference_decoder_through_resize_equals_load_image(tmp_path):
    for i, (samp, size, keep) in enumerate(itertools.product((0, 2), ((320, 320), (640, 640)), (False, True))):
        p = tmp_path / f"{i}.jpg"
        p.write_bytes(_encode(_image(45, 29, 20 + i), samp, quality=85))
        ref, sc = load_image(str(p), size, keep, True)
        info = jpeg.parse(p.read_bytes())
        (nw, nh), sc2 = resample.letterbox_size((info.height, info.width), size, keep)
        canvas = np.zeros(size + (3,), np.uint8)
        canvas[:nh, :nw] = resample.resize(jpeg_ref.decode(info), (nw, nh))
        assert sc == sc2
        np.testing.assert_array_equal(canvas, ref)
