"""Crafted JPEG streams on the host (no GPU): files that Pillow's encoder never writes (tests/jpeg_write.py,
tests/jpeg_crafted.py) decode equal to PIL through jpeg.parse + the numpy reference decoder, each regime is asserted from
the reference side, and jpeg.parse keeps its contract (a JpegInfo or Fallback, nothing else) under header mutations."""
import io
import pathlib
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import jpeg_crafted  # noqa: E402
import jpeg_ref  # noqa: E402
import jpeg_write  # noqa: E402

from object_detector_amd import jpeg, resample  # noqa: E402
from object_detector_amd.imageio import load_image  # noqa: E402


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _pillow_jpeg(a, **kw):
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG", **kw)
    return f.getvalue()


def test_writer_standard_tables_are_pillows():
    """The writer's Annex K tables give the decode tables of the ones Pillow writes by default."""
    info = jpeg.parse(_pillow_jpeg(jpeg_crafted.picture(32, 32, 0)))
    for i, key in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):  # (class, slot) of info.huff rows 0..3
        np.testing.assert_array_equal(info.huff[i], jpeg.huff_table(*jpeg_write.STD_HUFF[key], key[0] == 0))


def test_writer_never_assigns_the_all_ones_code():
    for counts, symbols in list(jpeg_write.STD_HUFF.values()) + [jpeg_write.LONG_AC, jpeg_write.LONG_DC,
                                                                 jpeg_crafted.FLAT4_DC, jpeg_crafted.MIXED_AC]:
        for code, ln in jpeg_write.code_map(counts, symbols).values():
            assert code != (1 << ln) - 1
    assert {ln for _, ln in jpeg_write.code_map(*jpeg_write.LONG_AC).values()} == {1, 2, 3, 4, 5, 6, 7, 16}
    assert sum(ln == 16 for _, ln in jpeg_write.code_map(*jpeg_write.LONG_AC).values()) == 162


@pytest.mark.parametrize("name", jpeg_crafted.GROUPS)
def test_crafted_files_decode_equal_to_pil(name):
    """Ties the writer to libjpeg, and PIL (the device tests' reference) to a second, independent decoder."""
    for case, data in jpeg_crafted.group(name).items():
        ref = _pil(data)  # PIL refusing a crafted file means the writer is wrong
        info = jpeg.parse(data)
        np.testing.assert_array_equal(jpeg_ref.decode(info), ref, err_msg=case)


def test_coefficient_files_round_trip():
    """What encode_blocks was given is what the reference entropy decode returns."""
    for s, kind in enumerate(("only63", "only49", "full", "alternating")):
        files = jpeg_crafted.group("coef")
        np.testing.assert_array_equal(jpeg_ref.coefficients(jpeg.parse(files[f"{kind}_grey"])),
                                      jpeg_crafted.coef_blocks(kind, 12, s), err_msg=kind)
        np.testing.assert_array_equal(jpeg_ref.coefficients(jpeg.parse(files[f"{kind}_420"])),
                                      jpeg_crafted.coef_blocks(kind, 24, 10 + s), err_msg=kind)


def test_regime_long_blocks():
    """Every block is longer than a subsequence, so some subsequences hold no block start."""
    for case, data in jpeg_crafted.group("long").items():
        info = jpeg.parse(data)
        starts = jpeg_ref.scan(info).starts
        subs = info.subsequences()
        per_sub = [np.count_nonzero((starts >= lo) & (starts < hi)) for lo, hi in subs[:, :2]]
        assert min(per_sub) == 0, case
        assert len(info.stream) * 8 / info.n_blocks > jpeg.SUB_BITS, case
        if info.restart == 0:
            assert np.diff(starts).min() > jpeg.SUB_BITS, case
    assert len(jpeg.parse(jpeg_crafted.group("long")["long_grey"]).subsequences()) >= 20


def test_regime_extreme_magnitudes():
    for case, data in jpeg_crafted.group("extreme").items():
        sc = jpeg_ref.scan(jpeg.parse(data))
        if case.endswith("q1"):
            assert (sc.dc_cat, sc.ac_cat) == (11, 10), case
            assert np.abs(np.diff(sc.coef[:, 0].astype(int))).max() == 2040 and np.abs(sc.coef[:, 1:]).max() >= 512, case
        else:
            assert (sc.dc_cat, sc.ac_cat) == (10, 9), case


def test_regime_no_eob_and_zrl():
    files = jpeg_crafted.group("coef")
    for case in ("full_grey", "full_420", "alternating_grey", "alternating_420", "only63_grey", "only63_420"):
        assert np.count_nonzero(jpeg_ref.scan(jpeg.parse(files[case])).coef[:, 63]) >= 6, case
    for case in ("only63_grey", "only63_420", "only49_grey", "only49_420"):
        sc = jpeg_ref.scan(jpeg.parse(files[case]))
        assert sc.zrl_run == 3, case
        assert np.count_nonzero(sc.coef[:, 1:]) == len(sc.coef), case  # one AC coefficient per block


def test_regime_distinct_tables():
    for case, data in jpeg_crafted.group("tables").items():
        info = jpeg.parse(data)
        for a, b in ((0, 2), (0, 4), (2, 4), (1, 3), (1, 5), (3, 5)):  # DC tables, then AC tables, pairwise
            assert not np.array_equal(info.huff[a], info.huff[b]), case
        assert not np.array_equal(info.quant[1], info.quant[2]) and not np.array_equal(info.quant[0], info.quant[1]), case
    info = jpeg.parse(jpeg_crafted.group("tables")["tables_422"])
    assert info.restart == 3 and info.n_seg == 3 and info.samp[0] == (2, 1) and (info.width, info.height) == (37, 19)
    info = jpeg.parse(jpeg_crafted.group("tables")["tables_444"])
    assert info.restart == 3 and info.mcux % 3 != 0 and info.n_seg == 5  # intervals that straddle MCU rows


def test_regime_header_forms():
    files = jpeg_crafted.group("headers")
    assert files["dqt16"].count(b"\xff\xdb") == 2 and b"\xff\xdb\x00\x83\x10" in files["dqt16"]
    assert files["one_segment"].count(b"\xff\xc4") == 1 and files["one_segment"].count(b"\xff\xdb") == 1
    assert files["tables_after_sof"].index(b"\xff\xc0") < files["tables_after_sof"].index(b"\xff\xdb")
    assert b"\xff\xfe" in files["extras"] and b"\xff\xe5" in files["extras"]
    assert files["fill"].count(b"\xff\xff\xd0") == 1 and files["fill"].endswith(b"\xff\xff\xff\xd9")
    info = jpeg.parse(files["dri_past_end"])
    assert info.restart > info.mcux * info.mcuy and info.n_seg == 1
    assert jpeg.parse(files["dri_zero"]).restart == 0 and b"\xff\xdd\x00\x04\x00\x00" in files["dri_zero"]
    ordinary = jpeg.parse(files["one_segment"])
    for case in ("dqt16", "tables_after_sof", "extras", "dri_past_end", "dri_zero"):
        info = jpeg.parse(files[case])
        np.testing.assert_array_equal(info.stream, ordinary.stream, err_msg=case)
        np.testing.assert_array_equal(info.quant, ordinary.quant, err_msg=case)


def test_sync_rounds_of_flat_shared_table_images():
    """Every block of a flat image coded with one shared table pair is the same 20 bits (DC category 0 at 4 bits, EOB
    at 16), so a subsequence's guess "block 0 of the MCU" is wrong in the block index and nothing in the bits corrects
    it: the right state only arrives by propagation from subsequence 0.  The model (jpeg_ref.sync_rounds) at 400 x 304:
    4:2:0 56 subsequences, 56 rounds; 4:2:2 75 subsequences, 75 rounds; grey 38 subsequences, 38 rounds (one block per
    MCU, but a subsequence starts 4 bits into a block and the periodic bit string never re-aligns the guess)."""
    files = jpeg_crafted.group("flat")
    for case in ("flat_420", "flat_422", "flat_grey"):
        info = jpeg.parse(files[case])
        assert np.all(np.diff(jpeg_ref.scan(info).starts) == 20), case
        n = len(info.subsequences())
        rounds = jpeg_crafted.model_rounds("flat", case)
        assert n >= 32 and n / 2 <= rounds <= n + 1, (case, n, rounds)


def test_sync_model_ends_on_the_sequential_decode():
    """The model's final exit states are states the sequential decode passes through: every exit sits on a symbol
    boundary of the right block (checked at exits that fall on a block start), so the model is a model of this
    decoder and not of another one."""
    seen = 0
    for name, case in (("long", "long_444"), ("flat", "flat_420"), ("tables", "tables_422"), ("extreme", "extreme_420_q1"),
                       ("coef", "full_420"), ("geometry", "422_std_2000x1")):
        info = jpeg.parse(jpeg_crafted.group(name)[case])
        starts = jpeg_ref.scan(info).starts.tolist()
        subs = info.subsequences()
        rounds, ex = jpeg_ref.sync_states(info)
        assert rounds <= len(subs), case  # converged, not cut off
        for j, (pos, c, k) in enumerate(ex):
            if subs[j, 1] == subs[j, 2]:
                continue  # the last subsequence of an interval runs into the padding
            g = np.searchsorted(starts, pos, side="right") - 1  # the block that holds bit `pos`
            assert c == g % info.bpm, (case, j)
            assert (k == 0) == (starts[g] == pos), (case, j)
            seen += k == 0
    assert seen >= 10


def test_sync_rounds_model_on_pillow_files():
    """The model on ordinary files: one round when there is one subsequence, and never more than one per subsequence
    plus the confirming one."""
    for samp, (w, h) in ((2, (8, 8)), (0, (64, 48)), (1, (120, 90))):
        info = jpeg.parse(_pillow_jpeg(jpeg_crafted.picture(w, h, w), subsampling=samp, quality=90))
        n = len(info.subsequences())
        rounds = jpeg_ref.sync_rounds(info)
        assert 1 <= rounds <= n + 1 and (n > 1 or rounds == 1)


def test_luma_1x2_takes_the_device_route():
    for (w, h), data in zip(jpeg_crafted.H1V2_SIZES, jpeg_crafted.group("h1v2").values()):
        info = jpeg.parse(data)
        im = Image.open(io.BytesIO(data))
        assert (info.width, info.height) == im.size == (w, h)
        assert [(hs, vs) for _, hs, vs, _ in im.layer] == info.samp == [(1, 2), (1, 1), (1, 1)]
        assert (info.mcux, info.mcuy, info.bpm) == (-(-w // 8), -(-h // 16), 4)
        for ci, (_, _, _, tq) in enumerate(im.layer):
            np.testing.assert_array_equal(info.quant[ci], np.asarray(im.quantization[tq]))


def test_all_ones_huffman_code_falls_back_as_libjpeg_refuses():
    """A complete table (sixteen 4-bit DC codes: 1111 is assigned): libjpeg refuses it, so the file must not take the
    device route either.  The same table with one code fewer is fine on both routes."""
    a = jpeg_crafted.picture(24, 16, 6)
    full = (bytes([0, 0, 0, 16] + [0] * 12), bytes(range(16)))
    data = jpeg_write.encode_pixels(a, (2, 2), htabs={**jpeg_write.STD_HUFF, (0, 1): full}, strict=False)
    with pytest.raises(jpeg.Fallback):
        jpeg.parse(data)
    with pytest.raises(OSError):
        Image.open(io.BytesIO(data)).load()
    with pytest.raises(jpeg.Fallback):
        jpeg.huff_table(bytes([1, 1, 1, 1, 2] + [0] * 11), bytes(range(6)), False)  # 0 10 110 1110 11110 11111
    ok = (bytes([0, 0, 0, 15] + [0] * 12), bytes(range(15)))
    data = jpeg_write.encode_pixels(a, (2, 2), htabs={**jpeg_write.STD_HUFF, (0, 1): ok})
    np.testing.assert_array_equal(jpeg_ref.decode(jpeg.parse(data)), _pil(data))


def test_odd_16_bit_dqt_falls_back():
    """A DQT that announces 16-bit entries over an odd number of table bytes used to escape as ValueError."""
    data = jpeg_crafted.group("headers")["one_segment"]
    for n in (127, 1, 63, 129):
        extra = b"\xff\xdb" + (n + 3).to_bytes(2, "big") + b"\x13" + bytes([5]) * n  # Pq = 1, slot 3, n table bytes
        with pytest.raises(jpeg.Fallback):
            jpeg.parse(data[:2] + extra + data[2:])
    extra = b"\xff\xdb\x00\x83\x13" + bytes([0, 5]) * 64  # the well-formed one is accepted (slot 3 is not used)
    np.testing.assert_array_equal(jpeg_ref.decode(jpeg.parse(data[:2] + extra + data[2:])), _pil(data))


TALL = [(8, 1500), (8, 801), (8, 800), (10, 1001), (1, 101), (1, 100), (3, 400)]  # (w, h) around height = 100 * width


@pytest.mark.parametrize("dst_wh", [(96, 96), (320, 320), (8, 96), (1, 96), (20, 900), (96, 2000)])
def test_resample_pass_order_of_tall_narrow_images(dst_wh):
    """Image.resize runs the vertical pass first when height > 100 * width and the height shrinks; the 8-bit rounding
    between the passes makes the order visible, so resample.resize has to follow it."""
    for w, h in TALL:
        a = np.random.default_rng(w * h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(a).resize(dst_wh, Image.BILINEAR))
        np.testing.assert_array_equal(resample.resize(a, dst_wh), ref, err_msg=f"{w}x{h}")
    a = np.random.default_rng(1).integers(0, 256, (1500, 8, 3), dtype=np.uint8)
    first_h = resample._pass(resample._pass(a, 1, 96), 0, 96)
    assert np.any(first_h != resample.resize(a, (96, 96)))  # the cases above can tell the two orders apart


def test_tall_crafted_file_through_resize_equals_load_image(tmp_path):
    p = tmp_path / "tall.jpg"
    p.write_bytes(jpeg_crafted.group("geometry")["grey_std_8x1500"])
    info = jpeg.parse(p.read_bytes())
    img = jpeg_ref.decode(info)
    for size in ((96, 96), (320, 320)):
        for keep in (False, True):
            ref, sc = load_image(str(p), size, keep, True)
            (nw, nh), sc2 = resample.letterbox_size((info.height, info.width), size, keep)
            canvas = np.zeros(size + (3,), np.uint8)
            canvas[:nh, :nw] = resample.resize(img, (nw, nh))
            assert sc == sc2
            np.testing.assert_array_equal(canvas, ref, err_msg=f"{size} {keep}")


def _sos_header_end(data):
    i = 2
    while True:
        assert data[i] == 0xFF
        ln = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xDA:
            return i + 2 + ln
        i += 2 + ln


def test_parse_contract_under_header_mutations():
    """20 000 seeded mutations (1 to 3 byte changes between SOI and the end of the SOS header, a fifth also truncated)
    of four files: only Fallback escapes parse / subsequences, and what is accepted stays inside its own ranges."""
    a = jpeg_crafted.picture(61, 43, 8)
    bases = [_pillow_jpeg(a, subsampling=2, quality=80), _pillow_jpeg(a, subsampling=0, quality=90, optimize=True),
             _pillow_jpeg(a, subsampling=1, quality=70, restart_marker_blocks=3), _pillow_jpeg(a[..., 0], quality=85)]
    ends = [_sos_header_end(b) for b in bases]
    rng = np.random.default_rng(2024)
    accepted = 0
    for n in range(20000):
        base, end = bases[n % 4], ends[n % 4]
        data = bytearray(base)
        for pos in rng.integers(2, end, int(rng.integers(1, 4))):
            data[pos] = int(rng.integers(0, 256))
        if n % 5 == 0:
            del data[int(rng.integers(2, len(data))):]
        try:
            info = jpeg.parse(bytes(data))
            subs = info.subsequences()
        except jpeg.Fallback:
            continue
        accepted += 1
        bits = len(info.stream) * 8
        assert info.huff.shape == (6, jpeg.HUFF_INTS) and info.huff.dtype == np.int32
        assert info.quant.shape == (3, 64)
        assert len(subs) >= 1 and subs.shape[1] == jpeg.SUB_INTS
        assert np.all((0 <= subs[:, 0]) & (subs[:, 0] <= subs[:, 1]) & (subs[:, 1] <= subs[:, 2]) & (subs[:, 2] <= bits))
        assert np.all((0 <= subs[:, 3]) & (subs[:, 3] < subs[:, 4]) & (subs[:, 4] <= info.n_blocks))
        assert info.n_blocks == info.mcux * info.mcuy * info.bpm and 1 <= info.bpm <= 6
    assert 2000 < accepted < 18000  # the mutations reach both outcomes
