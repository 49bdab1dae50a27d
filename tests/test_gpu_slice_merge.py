"""GPU: od_slice_merge (the merge of sliced inference) against the numpy restatement tests/slice_ref.py, bit for bit: kept
(tile, flat), class, confidence bits, box bits, counts and padding, on the generated scenarios of slice_ref.scenario (whose
conditions tests/test_slicing_host.py checks on the reference).  Every output is a view inside a sentinel-filled allocation
whose guards must stay untouched; nothing here has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lattice_ref as L
import slice_ref
import tta_ref

pytestmark = pytest.mark.gpu

F = np.float32
THR, MAX_DET = 0.45, 200


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ctx(cuda):
    from object_detector_amd import _lib
    from object_detector_amd.net import Context
    ctx = Context.get(cuda)
    return _lib, ctx.lib, ctx.handle


@functools.lru_cache(maxsize=None)
def _scenario(name):
    """The scenario and, per image, its surviving candidates: computed once, shared by every (strict, vote_iou) case."""
    sc = slice_ref.scenario(name)
    cands = []
    for g in range(sc["G"]):
        lists, edge, aff = slice_ref.image_lists(sc, g)
        cands.append(slice_ref.candidates(lists, sc["NC"], edge, aff, sc["edge_lo"], sc["edge_hi"]))
    return sc, cands


def _check(out, src, kc, ref, g, what):
    n = len(ref["cls"])
    assert int(kc[g]) == n, (what, g, int(kc[g]), n)
    row = out[g]
    assert int(row[:1].view(np.int32)[0]) == n, (what, g)
    rec = row[1:].reshape(MAX_DET, 6).view(np.uint32)
    assert np.array_equal(src[g, :n], ref["src"]), (what, g)
    assert np.array_equal(rec[:n, 0].view(np.int32), ref["cls"]), (what, g)
    assert np.array_equal(rec[:n, 1], ref["conf_bits"]), (what, g)
    assert np.array_equal(rec[:n, 2:6], ref["boxes"].view(np.uint32)), (what, g)
    assert (rec[n:, 0].view(np.int32) == -1).all() and (rec[n:, 1:] == 0).all() and (src[g, n:] == -1).all(), (what, g)
    return n


def _device(cuda, sc):
    """The inputs as byte views in the middle of poisoned allocations (16-byte aligned)."""
    return {k: L.poisoned(np.ascontiguousarray(sc[k]).view(np.uint8).reshape(-1), cuda)
            for k in ("keys", "counts", "boxes", "tiles", "edges")}


def _merge(cuda, sc, dev, strict, vote_iou, out, src, kc, ws, ws_bytes):
    _lib, lib, h = _ctx(cuda)
    _lib.check(lib.od_slice_merge(h, dev["keys"].data_ptr(), dev["counts"].data_ptr(), dev["boxes"].data_ptr(),
                                  dev["tiles"].data_ptr(), dev["edges"].data_ptr(), sc["G"], sc["T"], sc["P"], sc["NC"], sc["K"],
                                  sc["edge_lo"], sc["edge_hi"], THR, strict, MAX_DET, float(vote_iou), out.t.data_ptr(),
                                  None if src is None else src.t.data_ptr(), kc.t.data_ptr(), ws.t.data_ptr(), ws_bytes,
                                  _stream()), "od_slice_merge")
    torch.cuda.synchronize()


@pytest.mark.parametrize("vote_iou", [0.0, 0.5])
@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("name", list(slice_ref.SCENARIOS))
def test_slice_merge_equals_reference(cuda, name, strict, vote_iou):
    """Three consecutive calls on one workspace that is filled with a different byte before each; src NULL gives the same
    block."""
    _lib, lib, h = _ctx(cuda)
    sc, cands = _scenario(name)
    G, T, K = sc["G"], sc["T"], sc["K"]
    dev = _device(cuda, sc)
    ws_bytes = lib.od_slice_merge_workspace_bytes(G, T, K)
    assert ws_bytes > 0
    ws = L.Guarded((ws_bytes,), torch.uint8, cuda)
    out = L.Guarded((G, 1 + 6 * MAX_DET), torch.float32, cuda)
    src = L.Guarded((G, MAX_DET, 2), torch.int32, cuda)
    kc = L.Guarded((G,), torch.int32, cuda)
    results = []
    for rep in range(3):
        ws.t.fill_((0x00, 0xFF, 0x5A)[rep])  # nothing may carry over from call to call, or depend on what was there
        out.t.fill_(float("nan")), src.t.fill_(12345), kc.t.fill_(-9)
        _merge(cuda, sc, dev, strict, vote_iou, out, src, kc, ws, ws_bytes)
        ws.check("workspace")
        results.append((out.numpy("out").copy(), src.numpy("src").copy(), kc.numpy("keep_count").copy()))
    for r in results[1:]:
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r, results[0])), "calls differ"
    o, s, n = results[0]
    kept = 0
    for g in range(G):
        lists, edge, aff = slice_ref.image_lists(sc, g)
        ref = slice_ref.merge_image(lists, sc["NC"], K, edge, aff, sc["edge_lo"], sc["edge_hi"], THR, bool(strict), MAX_DET,
                                    vote_iou, cands=cands[g])
        kept += _check(o, s, n, ref, g, name)
    assert (kept == 0) == (name == "all_empty")
    out.t.fill_(float("nan"))
    _merge(cuda, sc, dev, strict, vote_iou, out, None, kc, ws, ws_bytes)
    assert np.array_equal(out.numpy("out").view(np.uint32), o.view(np.uint32))
    for k in ("keys", "counts", "boxes", "tiles", "edges"):
        assert np.array_equal(dev[k].cpu().numpy(), sc[k].view(np.uint8).reshape(-1)), k


@pytest.mark.parametrize("T", [1, 4])
def test_tiles_equal_tta_merge_with_views(cuda, T):
    """Tiles that are the whole image (affine row (0, 0, 1, 1), no interior side, the rule disabled) are unflipped views:
    od_slice_merge on rows g * T + t and od_tta_merge on the same lists passed as V = T views give the same record block,
    sources and keep counts, word for word.  G = B = 2; K = 200 is no multiple of 64 (a partial wave in the compaction);
    the boxes lie in [0, 1], where the tiles' clamp changes nothing."""
    _lib, lib, h = _ctx(cuda)
    G, K, P, NC = 2, 200, 4200, 20
    rng = np.random.default_rng(L.seed_of("tiles_as_views", T))
    keys, boxes = np.zeros((G * T, K), np.uint64), np.zeros((G * T, P, 4), F)
    counts = np.array([K if r % 3 == 0 else int(rng.integers(1, K)) for r in range(G * T)], np.int32)
    for r in range(G * T):
        keys[r], boxes[r] = slice_ref.make_row(rng, K, P, NC, int(counts[r]), quantise=r % 2 == 0)
    assert boxes.min() >= 0 and boxes.max() <= 1
    sc = {"G": G, "T": T, "K": K, "P": P, "NC": NC, "keys": keys, "counts": counts, "boxes": boxes, "edge_lo": -1.0,
          "edge_hi": 2.0, "tiles": np.tile(np.array([0, 0, 1, 1], F), (G * T, 1)), "edges": np.zeros(G * T, np.int32)}
    outs = []
    for which in ("slice", "tta"):
        out = L.Guarded((G, 1 + 6 * MAX_DET), torch.float32, cuda)
        src = L.Guarded((G, MAX_DET, 2), torch.int32, cuda)
        kc = L.Guarded((G,), torch.int32, cuda)
        if which == "slice":
            nb = lib.od_slice_merge_workspace_bytes(G, T, K)
            ws = L.Guarded((nb,), torch.uint8, cuda)
            _merge(cuda, sc, _device(cuda, sc), 0, 0.5, out, src, kc, ws, nb)
        else:
            nb = lib.od_tta_merge_workspace_bytes(G, T, K)
            ws = L.Guarded((nb,), torch.uint8, cuda)
            # view t = rows t, T + t, ...: [B, ...] arrays of their own, as od_tta_view takes them
            dev = [{k: L.poisoned(np.ascontiguousarray(sc[k][t::T]).view(np.uint8).reshape(-1), cuda)
                    for k in ("keys", "counts", "boxes")} for t in range(T)]
            desc = (_lib.TtaView * T)()
            for t, d in enumerate(dev):
                desc[t] = _lib.TtaView(d["keys"].data_ptr(), d["counts"].data_ptr(), d["boxes"].data_ptr(), P, 0)
            _lib.check(lib.od_tta_merge(h, desc, T, G, NC, K, THR, 0, MAX_DET, 0.5, out.t.data_ptr(), src.t.data_ptr(),
                                        kc.t.data_ptr(), ws.t.data_ptr(), nb, _stream()), "od_tta_merge")
            torch.cuda.synchronize()
        ws.check("workspace")
        outs.append((out.numpy("out").view(np.uint32), src.numpy("src").view(np.uint32), kc.numpy("kc").view(np.uint32)))
    assert all(np.array_equal(a, b) for a, b in zip(*outs)) and (outs[0][2] > 0).all()


def test_slice_merge_rejects_bad_arguments(cuda):
    _lib, lib, h = _ctx(cuda)
    t = torch.zeros(1024, dtype=torch.int64, device=cuda)
    assert lib.od_slice_merge_workspace_bytes(1, 17, 4) == 0 and lib.od_slice_merge_workspace_bytes(1, 1, 2048) == 0
    assert lib.od_slice_merge_workspace_bytes(0, 1, 4) == 0 and lib.od_slice_merge_workspace_bytes(1, 0, 4) == 0
    n = lib.od_slice_merge_workspace_bytes(1, 2, 4)
    ws = torch.zeros(n, dtype=torch.uint8, device=cuda)
    p = t.data_ptr()
    for T, K, nbytes, keys, msg in ((17, 4, n, p, "outside 1..16"), (0, 4, n, p, "outside 1..16"), (2, 2048, n, p, "K <= 1024"),
                                    (2, 4, n - 1, p, "workspace"), (2, 4, n, None, "null")):
        with pytest.raises(_lib.OdError, match=msg):
            _lib.check(lib.od_slice_merge(h, keys, p, p, p, p, 1, T, 8, 20, K, 0.01, 0.99, 0.45, 0, 4, 0.5, p, None, p,
                                          ws.data_ptr(), nbytes, _stream()), "od_slice_merge")
