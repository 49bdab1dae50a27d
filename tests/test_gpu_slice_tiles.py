"""GPU: od_tiles_resize (the tile cutter of sliced inference) against tests/slice_ref.tile_pixels, byte for byte.  The blob is
a view inside a poisoned allocation, the output and the workspace are views inside sentinel-filled ones whose guards must stay
untouched; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import lattice_ref as L
import slice_ref
from object_detector_amd import resample, slicing

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ctx(cuda):
    from object_detector_amd import _lib
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return _lib, ctx.lib, ctx.handle


def _pack(_lib, images, rect_lists, H, W, pad=0, shift=0):
    """-> (descs, blob u8): every image once in the blob (rows `pad` bytes apart beyond their pixels, the first image `shift`
    bytes past a 16-byte boundary; the padding holds 255), one descriptor per rectangle, tables 16-byte aligned."""
    N = sum(len(r) for r in rect_lists)
    descs = (_lib.TileDesc * N)()
    parts, off, tables, n = [], 0, {}, 0

    def put(a, lead=0):
        nonlocal off
        off = (off + 15) // 16 * 16 + lead
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        parts.append((off, a))
        off += a.nbytes
        return parts[-1][0]

    def table(n_in, n_out):
        if (n_in, n_out) not in tables:
            t = resample.table(n_in, n_out)
            tables[n_in, n_out] = (put(t), t.shape[1] - 2)
        return tables[n_in, n_out]

    for img, rects in zip(images, rect_lists):
        h, w = img.shape[:2]
        rows = np.full((h, 3 * w + pad), 255, np.uint8)
        rows[:, :3 * w] = img.reshape(h, 3 * w)
        src = put(rows, shift)
        for x0, y0, x1, y1 in np.asarray(rects).tolist():
            d = descs[n]
            n += 1
            d.src_off, d.pitch, d.src_w, d.src_h = src, 3 * w + pad, w, h
            d.x0, d.y0, d.x1, d.y1 = x0, y0, x1, y1
            d.hcoef_off, d.hk = table(x1 - x0, W)
            d.vcoef_off, d.vk = table(y1 - y0, H)
    blob = np.full(off, 255, np.uint8)
    for o, a in parts:
        blob[o:o + a.nbytes] = a
    return descs, blob


GRID = slicing.SliceGrid(2, 2, 0.2, True)


def _case(name):
    rng = np.random.default_rng(L.seed_of("tiles", name))

    def img(h, w):
        return rng.integers(0, 255, (h, w, 3), dtype=np.uint8)  # 255 is the poison around the blob and in the row padding
    if name == "200x150":  # up- and down-scaling in one call: the tiles grow to 96 x 96, the full view shrinks
        ims, grids, size, kw = [img(150, 200)], [GRID], (96, 96), {}
    elif name == "copy":  # one tile = the whole 96 x 96 image: both passes are skipped
        ims, grids, size, kw = [img(96, 96)], [slicing.SliceGrid(1, 1, 0.2, False)], (96, 96), {}
    elif name == "33x50_pitch150":  # 50 wide, 33 high: rows 150 bytes apart
        ims, grids, size, kw = [img(33, 50)], [GRID], (96, 96), {}
    elif name == "padded_rows_odd_offset":  # pitch 3 * 77 + 5, the image 3 bytes past a 16-byte boundary
        ims, grids, size, kw = [img(61, 77)], [GRID], (64, 96), {"pad": 5, "shift": 3}
    elif name == "two_sources":
        ims, grids, size, kw = [img(150, 200), img(97, 333)], [GRID, GRID], (96, 96), {}
    elif name == "one_pass_only":  # tiles as wide as the output (horizontal pass skipped), and as high (vertical skipped)
        ims, size, kw = [img(300, 96), img(64, 200)], (96, 64), {}
        grids = [slicing.SliceGrid(2, 1, 0.2, False), slicing.SliceGrid(1, 2, 0.2, False)]
    else:
        assert name == "64x6500_vertical_first"
        ims, grids, size, kw = [img(6500, 64)], [slicing.SliceGrid(1, 2, 0.2, True)], (96, 96), {}
    rects = [g.rects(im.shape[1], im.shape[0]) for g, im in zip(grids, ims)]
    return ims, rects, size, kw


CASES = ["200x150", "copy", "33x50_pitch150", "padded_rows_odd_offset", "two_sources", "one_pass_only", "64x6500_vertical_first"]


@pytest.mark.parametrize("name", CASES)
def test_tiles_resize_equals_reference(cuda, name):
    _lib, lib, h = _ctx(cuda)
    ims, rects, (W, H), kw = _case(name)
    want = np.concatenate([slice_ref.tile_pixels(im, r, (W, H)) for im, r in zip(ims, rects)])
    N = len(want)
    if name == "64x6500_vertical_first":
        assert all(resample.vertical_first((y1 - y0, x1 - x0), H) for x0, y0, x1, y1 in rects[0].tolist())
    if name == "one_pass_only":
        assert (rects[0][:, 2] - rects[0][:, 0] == W).all() and (rects[1][:, 3] - rects[1][:, 1] == H).all()
    descs, blob = _pack(_lib, ims, rects, H, W, **kw)
    wsb = C.c_longlong(-1)
    _lib.check(lib.od_tiles_workspace_plan(descs, N, H, W, C.byref(wsb)), "od_tiles_workspace_plan")
    assert wsb.value >= 0 and (name != "copy" or wsb.value == 0)
    ws = L.Guarded((max(wsb.value, 16),), torch.uint8, cuda)
    blob_d = L.poisoned(blob, cuda)
    descs_d = torch.from_numpy(np.frombuffer(descs, np.uint8).copy()).to(cuda)
    out = L.Guarded((N + 2, H, W, 3), torch.uint8, cuda)
    results = []
    for fill in (0x00, 0xFF, 0x5A):  # nothing may carry over from call to call, or depend on what the workspace held
        ws.t.fill_(fill)
        out.t.fill_(L.SENTINEL)
        _lib.check(lib.od_tiles_resize(h, descs, descs_d.data_ptr(), N, blob_d.data_ptr(), blob.nbytes, ws.t.data_ptr(),
                                       wsb.value, out.t.data_ptr(), H, W, _stream()), "od_tiles_resize")
        torch.cuda.synchronize()
        ws.check("workspace")
        results.append(out.numpy("out").copy())
    for r in results:
        assert np.array_equal(r[:N], want), name
        assert (r[N:] == L.SENTINEL).all(), "rows past N were written"
    assert np.array_equal(blob_d.cpu().numpy(), blob)


def test_batch_decoder_tiles_route(cuda):
    """BatchDecoder.run_tiles (what predict(image_decode="device") runs with slices): the same tiles, row g*T + t."""
    from object_detector_amd.devdecode import BatchDecoder
    rng = np.random.default_rng(3)
    ims = [rng.integers(0, 256, (150, 200, 3), dtype=np.uint8), rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)]
    out = L.Guarded((12, 96, 96, 3), torch.uint8, cuda)
    dec = BatchDecoder(cuda)
    for _rep in range(2):
        out.t.fill_(L.SENTINEL)
        sizes = dec.run_tiles(ims, GRID, out.t)
        torch.cuda.synchronize()
        assert sizes == [(200, 150), (96, 96)]
        got = out.numpy("tiles")
        want = np.concatenate([slice_ref.tile_pixels(im, GRID.rects(im.shape[1], im.shape[0]), (96, 96)) for im in ims])
        assert np.array_equal(got[:10], want) and (got[10:] == L.SENTINEL).all()


def test_tiles_resize_rejects_bad_arguments(cuda):
    _lib, lib, h = _ctx(cuda)
    ims, rects, (W, H), kw = _case("200x150")
    descs, blob = _pack(_lib, ims, rects, H, W)
    N = len(descs)
    wsb = C.c_longlong()
    _lib.check(lib.od_tiles_workspace_plan(descs, N, H, W, C.byref(wsb)), "od_tiles_workspace_plan")
    assert wsb.value > 0
    ws = torch.zeros(wsb.value, dtype=torch.uint8, device=cuda)
    blob_d = torch.from_numpy(blob).to(cuda)
    descs_d = torch.from_numpy(np.frombuffer(descs, np.uint8).copy()).to(cuda)
    out = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=cuda)

    def call(d=descs, blob_ptr=blob_d.data_ptr(), blob_bytes=blob.nbytes, ws_ptr=ws.data_ptr(), ws_bytes=wsb.value,
             out_ptr=out.data_ptr()):
        _lib.check(lib.od_tiles_resize(h, d, descs_d.data_ptr(), N, blob_ptr, blob_bytes, ws_ptr, ws_bytes, out_ptr, H, W,
                                       _stream()), "od_tiles_resize")

    call()
    torch.cuda.synchronize()
    for args, msg in (({"ws_bytes": wsb.value - 1}, "workspace too small"), ({"ws_ptr": None}, "null"),
                      ({"out_ptr": None}, "null"), ({"blob_ptr": None}, "null"),
                      ({"blob_bytes": int(descs[0].src_off) + 150 * 600 - 1}, "source out of bounds"),
                      ({"blob_bytes": int(descs[0].vcoef_off)}, "tables out of bounds")):
        with pytest.raises(_lib.OdError, match=msg):
            call(**args)
    for field, val in (("x1", 201), ("y1", 151), ("x0", -1), ("x0", 112), ("y0", 84)):
        bad = (_lib.TileDesc * N)()
        C.memmove(bad, descs, C.sizeof(descs))
        setattr(bad[0], field, val)
        with pytest.raises(_lib.OdError, match="rectangle outside the source"):
            call(d=bad)
        with pytest.raises(_lib.OdError, match="rectangle outside the source"):
            _lib.check(lib.od_tiles_workspace_plan(bad, N, H, W, C.byref(C.c_longlong())), "od_tiles_workspace_plan")
    bad = (_lib.TileDesc * N)()
    C.memmove(bad, descs, C.sizeof(descs))
    bad[0].pitch = 3 * 200 - 1
    with pytest.raises(_lib.OdError, match="source out of bounds"):
        call(d=bad)
    torch.cuda.synchronize()
