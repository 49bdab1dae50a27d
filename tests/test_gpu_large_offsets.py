"""Tensors whose element offsets pass 2^31: the 64-bit offset paths of the conv epilogues and of the kernels that read or
write pred / y / grad / conf [B, P, C].

Since 1024 classes are supported a prediction row has up to 1030 floats and [B, P, NC + 6] passes 2^31 elements at ordinary
batch sizes (640 x 640, batch 32).  The library has separate code for that -- conv_describe's `off32` sends a launch whose
output offsets do not fit 31 bits to the run-time epilogue, which forms them in 64 bits; every row kernel casts by hand --
and this file is what executes it.

Section 1, conv OUTPUT offsets.  One arena (a single uint8 allocation of 10 GiB + 128 MiB filled with a poison byte) is viewed
as f16 or f32; the small lattice problem of test_gpu_conv_epilogue_variants.py (B = 3, 10 x 10, Cin 64) places its images in
it through out_batch_stride / out_pix_stride alone.  Every case asserts (a) the written rows equal the once-rounded float64
reference (tests/lattice_ref.py), (b) every other byte of the arena still holds the poison, checked on the device in 256-MiB
chunks, and (c) the kernel the plan resolved to: the compiled policy while `off32` holds, the run-time instantiation (-1)
beyond.  d.out points 64 MiB into the arena, so an offset truncated to 32 unsigned bits lands inside it and is seen by (b).
The boundary cases sit on the smallest step the 16-byte stores allow (8 elements) on either side of each of the two
inequalities of `off32`: B * obs = 2^31 - 8 | 2^31 + 16, and a last element offset of 2^31 - 9 | 2^31 - 1 (the predicate counts
one past the end, so it already refuses 2^31 - 1: conservative by one element).  tests/test_large_offsets_host.py proves, without a GPU, which side every case is on and that all
it writes lies inside the arena.

Section 2, dense consumers.  The tensors are real (8 to 8.7 GiB each) and almost every row is dead -- an all-zero target row
for the loss (exactly zero gradient, no contribution), the far-below-threshold background of test_gpu_detect_tail.py for
detection -- so that the CPU oracle runs on a few thousand live rows: in image 0, in the 256-row blocks around element
2^31, well past it, and in the last 300 rows.  References and tolerances are those of the existing test of each kernel.

What the audit of the offset expressions found ("Size limits"): every kernel that indexes these tensors forms
the offset in 64 bits, or in 32 bits under a guard that makes that safe.  od_assign_atss and od_assign_tal share
write_owned_row with od_assign_anchors but form the row pointer `y + ((long long)b * P + p) * C` in a kernel of their own
(od_claim_encode, assign_common.h), and od_assign_tal reads pred through expressions of its own (od_tal_prior: `pred + row0 *
C`; od_tal_claims: `pred + (long long)b * P * C`), so each gets one call here.  One gap was closed in conv_describe: a
grouped launch checked the input extent of its FIRST segment only.
"""
import collections
import ctypes as C
import pathlib
import sys
import time

import numpy as np
import pytest
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import lattice_ref as L  # noqa: E402
import test_gpu_conv_epilogue_variants as V  # noqa: E402

E = V.E
NE8 = V.NE8
pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30
ARENA_BYTES = 10 * GiB + 128 * MiB
OUT_OFF = 64 * MiB           # d.out = arena + OUT_OFF
CHUNK = 256 * MiB            # the poison check reads the arena in pieces of this size
POISON = L.SENTINEL
LIM31 = 1 << 31
ALIGN = 8                    # elements: the epilogues store 16 bytes (8 f16) / 2 x 16 bytes (8 f32) per lane


def off32(B, obs, ops, hw_max, Cout):
    """conv_describe's predicate (csrc/conv_dispatch.hip), restated."""
    return obs >= 0 and ops >= 0 and B * obs < LIM31 and (B - 1) * obs + (hw_max - 1) * ops + Cout < LIM31


# ---- section 1: the cases ---------------------------------------------------------------------------------------------
# name, layer (B, H, W, Cin, Cout, k, stride, act, res, cfg), out_f32, obs, ops (elements), splitk, off32 (the side claimed)
OutCase = collections.namedtuple("OutCase", "name layer out_f32 obs ops splitk off32")

F32_E8 = ((3, 10, 10, 64, 208, 3, 1, None, "none", NE8), True)
F16_LAYERS = [((3, 10, 10, 64, cout, 3, 1, act, resm, cfg), False)
              for act, resm in (("leaky", "none"), ("leaky", "same"), ("elu", "up2")) for cfg, cout in ((7, 200), (NE8 + 1, 256))]
BOUNDARY_LAYERS = [F32_E8] + F16_LAYERS


def last_offset(layer, obs, ops):
    B, H, W, Cout = layer[0], layer[1], layer[2], layer[4]
    return (B - 1) * obs + (H * W - 1) * ops + Cout - 1


def strides_with_last_at(layer, last):
    """Interleaved images (B * obs <= ops: pixel q of image b starts at q * ops + b * obs) whose last element offset is
    exactly `last`: obs the smallest multiple of ALIGN >= Cout for which ops comes out a multiple of ALIGN."""
    B, hw, Cout = layer[0], layer[1] * layer[2], layer[4]
    obs = -(-Cout // ALIGN) * ALIGN
    while (last + 1 - Cout - (B - 1) * obs) % ((hw - 1) * ALIGN):
        obs += ALIGN
    ops = (last + 1 - Cout - (B - 1) * obs) // (hw - 1)
    assert B * obs <= ops
    return obs, ops


OBS_TIGHT = (LIM31 - 1) // 3 // ALIGN * ALIGN  # B = 3: the largest aligned obs with B * obs < 2^31


def _tag(layer, out_f32):
    cfg = layer[9]
    kern = f"e8mf{4 - (cfg - NE8)}" if cfg >= NE8 else f"cfg{cfg}"
    return f"{'f32' if out_f32 else 'f16'}-{layer[7] or 'linear'}-{layer[8]}-{layer[5]}x{layer[5]}-c{layer[4]}-{kern}"


def _boundary_cases():
    out = []
    for layer, f32 in BOUNDARY_LAYERS:
        t = _tag(layer, f32)
        # (i) conv_describe counts one past the last element: (B - 1) * obs + (HoWo - 1) * ops + Cout < 2^31.  Rows start on
        # multiples of 8 elements, so the last element offset is 7 mod 8: 2^31 - 9 is the largest the predicate admits, and
        # 2^31 - 1 -- every offset still fits 31 bits -- the first it refuses (conservative by one element, never unsafe)
        obs, ops = strides_with_last_at(layer, LIM31 - 1 - ALIGN)
        out.append(OutCase(f"last-under-{t}", layer, f32, obs, ops, 1, True))
        obs, ops = strides_with_last_at(layer, LIM31 - 1)
        out.append(OutCase(f"last-over-{t}", layer, f32, obs, ops, 1, False))
        # (ii) B * obs = 2^31 - 8, dense rows; one aligned step further B * obs = 2^31 + 16 while the last element stays far below
        out.append(OutCase(f"bobs-under-{t}", layer, f32, OBS_TIGHT, layer[4], 1, True))
        out.append(OutCase(f"bobs-over-{t}", layer, f32, OBS_TIGHT + ALIGN, layer[4], 1, False))
    return out


def _far_cases():
    out = []
    f16 = [(3, 10, 10, 64, 200, k, 1, "leaky", "same", 3) for k in (1, 3)] + \
          [(3, 10, 10, 64, 256, 3, 1, "leaky", "same", NE8 + 3), (3, 10, 10, 64, 256, 1, 1, "leaky", "same", NE8)]
    f32 = [(3, 10, 10, 64, 200, k, 1, None, "none", 3) for k in (1, 3)] + \
          [(3, 10, 10, 64, 208, 3, 1, None, "none", NE8 + 3), (3, 10, 10, 64, 208, 1, 1, None, "none", NE8)]
    for layers, is32, strides in ((f16, False, ((1 << 30) + 8, (1 << 31) + 8)), (f32, True, ((1 << 30) + 8,))):
        for obs in strides:
            for layer in layers:
                out.append(OutCase(f"far-obs{obs}-{_tag(layer, is32)}", layer, is32, obs, layer[4], 1, False))
    return out


BOUNDARY_CASES = _boundary_cases()
FAR_CASES = _far_cases()
SPLITK_CASE = OutCase("splitk-far", (3, 10, 10, 64, 200, 3, 1, "leaky", "same", 3), False, (1 << 30) + 8, 200, 2, False)
# out_pix_stride far larger than Cout.  With ops = 2^20 and obs = 100 * 2^20 (every image a block of its own) all offsets
# stay below 2^31: 300 * 2^20 = 3.1e8, so the compiled policies run.  For pixel * ops ALONE to pass 2^31 within 100 pixels
# ops must exceed 2^31 / 99 = 2.17e7: ops = 2^25 with the images interleaved (obs = 2^12), 99 * 2^25 = 3.3e9 elements.
PIX_LAYERS = [(3, 10, 10, 64, 200, 3, 1, "leaky", "same", 7), (3, 10, 10, 64, 256, 3, 1, "elu", "up2", NE8 + 2)]
PIX_CASES = [OutCase(f"pix-ops2^20-{_tag(l, False)}", l, False, 100 << 20, 1 << 20, 1, True) for l in PIX_LAYERS] + \
            [OutCase(f"pix-ops2^25-{_tag(l, False)}", l, False, 1 << 12, 1 << 25, 1, False) for l in PIX_LAYERS]
OUT_CASES = BOUNDARY_CASES + FAR_CASES + [SPLITK_CASE] + PIX_CASES
# the grouped launch: E8_GROUPED_CASE's shapes with f32 output, the caller's out_batch_stride for every segment
GROUPED_CASE = V.E8_GROUPED_CASE[:5] + (True, V.E8_GROUPED_CASE[6])
GROUPED_OBS = (1 << 30) + 8
GROUPED_SEG_GAP = 16 * MiB  # bytes between the segments' output pointers


def regions_of(oc):
    """What a case writes: [(first byte relative to the arena, B, pixels, Cout, obs, ops, element size)]."""
    B, H, W, Cout = oc.layer[0], oc.layer[1], oc.layer[2], oc.layer[4]
    return [(OUT_OFF, B, H * W, Cout, oc.obs, oc.ops, 4 if oc.out_f32 else 2)]


def grouped_regions():
    B, dims, _cin, Cout = GROUPED_CASE[:4]
    return [(OUT_OFF + i * GROUPED_SEG_GAP, B, h * w, Cout, GROUPED_OBS, Cout, 4) for i, (h, w) in enumerate(dims)]


def row_starts(region):
    """Element offset of every written row (one per image and pixel), relative to the region's first byte."""
    _, B, hw, _, obs, ops, _ = region
    return (np.arange(B, dtype=np.int64)[:, None] * obs + np.arange(hw, dtype=np.int64)[None, :] * ops).reshape(-1)


# ---- section 1: the arena ---------------------------------------------------------------------------------------------------
def need_free(cuda, nbytes, what):
    free, _total = torch.cuda.mem_get_info(cuda)
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes} bytes of device memory, {free} are free")


class _Arena:
    def __init__(self, cuda):
        self.cuda, self.t = cuda, None

    def get(self):
        if self.t is None:
            need_free(self.cuda, ARENA_BYTES + GiB, "the output arena")
            self.t = torch.full((ARENA_BYTES,), POISON, dtype=torch.uint8, device=self.cuda)
            assert self.t.data_ptr() % 256 == 0
        return self.t

    def free(self):
        self.t = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def arena(cuda):
    """The one arena of section 1: allocated and poisoned by the first case that asks, freed by the first test of section 2
    (the dense tensors need the room) or at the end of the module."""
    a = _Arena(cuda)
    yield a
    a.free()


@pytest.fixture(autouse=True)
def _wall_time_and_peak_memory(request):
    """One line per test for the record: wall time and torch.cuda.max_memory_allocated (shown with -s / -rA)."""
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"\n[large-offsets] {request.node.name}: {time.perf_counter() - t0:.2f} s, peak "
          f"{torch.cuda.max_memory_allocated() / GiB:.2f} GiB")


def poison_intact(t):
    """-> (ok, first bad byte offset or -1): every byte of t == POISON, read on the device in CHUNK pieces (the only
    temporaries are one bool per 8 bytes of a chunk)."""
    pat = int.from_bytes(bytes([POISON]) * 8, "little", signed=True)
    v = t.view(torch.int64)
    n = CHUNK // 8
    bad = torch.zeros((), dtype=torch.int64, device=t.device)
    for i in range(0, v.numel(), n):
        bad += (v[i:i + n] != pat).sum()
    if int(bad) == 0:
        return True, -1
    for i in range(0, v.numel(), n):
        nz = torch.nonzero(v[i:i + n] != pat)
        if nz.numel():
            return False, (i + int(nz[0])) * 8
    raise AssertionError("unreachable")


def _typed(arena_t, byte0, dtype):
    return arena_t[byte0:].view(dtype)


def read_rows(arena_t, region, dtype):
    """The rows a case wrote, gathered on the device through the same strides -> numpy [B, pixels, Cout]."""
    byte0, B, hw, Cout, obs, ops, _ = region
    return torch.as_strided(_typed(arena_t, byte0, dtype), (B, hw, Cout), (obs, ops, 1)).contiguous().cpu().numpy()


def restore_rows(arena_t, region):
    byte0, B, hw, Cout, obs, ops, es = region
    torch.as_strided(arena_t[byte0:], (B, hw, Cout * es), (obs * es, ops * es, 1)).fill_(POISON)


def check_background(arena, regions, what):
    """(b): with the written rows put back to poison, the WHOLE arena must hold poison.  A stray write leaves the arena
    dirty for the next case, so it is refilled before the failure is reported."""
    t = arena.get()
    for reg in regions:
        restore_rows(t, reg)
    ok, at = poison_intact(t)
    if not ok:
        t.fill_(POISON)
    assert ok, f"{what}: a byte outside the written rows changed, first at arena offset {at} (d.out is at {OUT_OFF})"


def compare(got, r, out_f32, what):
    if out_f32:
        L.assert_matches32(got.reshape(r.ref32.shape), r, what)
    else:
        L.assert_matches(got.reshape(r.ref16.shape), r, what)


@pytest.mark.parametrize("oc", OUT_CASES, ids=[c.name for c in OUT_CASES])
def test_conv_output_offsets(cuda, arena, oc):
    B, H, W, _cin, Cout = oc.layer[:5]
    assert off32(B, oc.obs, oc.ops, H * W, Cout) == oc.off32
    if oc.name.startswith("last-under"):  # both inequalities, the second one tight
        assert last_offset(oc.layer, oc.obs, oc.ops) == LIM31 - 1 - ALIGN and B * oc.obs < LIM31
    if oc.name.startswith("last-over"):  # the first inequality holds, the second fails by the one element it counts past the end
        assert last_offset(oc.layer, oc.obs, oc.ops) == LIM31 - 1 and B * oc.obs < LIM31
    if oc.name.startswith("bobs-under"):
        assert B * oc.obs < LIM31 <= B * (oc.obs + ALIGN) and last_offset(oc.layer, oc.obs, oc.ops) < LIM31
    t = arena.get()
    g, r = E.build_fwd(oc.layer, out_f32=oc.out_f32)
    keep = []
    try:
        d = V.conv_desc(cuda, g, oc.layer, keep, out_f32=oc.out_f32)
        d.out = t.data_ptr() + OUT_OFF
        d.out_batch_stride, d.out_pix_stride = oc.obs, oc.ops
        if oc.splitk != 1:  # the workspace of test_fwd_split_k; the finish kernel (od_conv_finish) writes the output
            keep.append(torch.empty(32 * B * H * W * Cout, dtype=torch.float32, device=cuda))
            d.splitk, d.splitk_workspace, d.splitk_workspace_bytes = oc.splitk, keep[-1].data_ptr(), keep[-1].numel() * 4
        name = V.run_plan(cuda, d, keep)
        (reg,) = regions_of(oc)
        got = read_rows(t, reg, torch.float32 if oc.out_f32 else torch.float16)
        check_background(arena, [reg], f"{name} {oc.name}")
        compare(got, r, oc.out_f32, f"{name} {oc.name}")
        # a split-K launch takes the run-time instantiation whatever its offsets
        V.check_name(name, *V.expected_name(oc.layer, out_f32=oc.out_f32, off32=oc.off32 and oc.splitk == 1))
    finally:
        del keep
        torch.cuda.empty_cache()


@pytest.mark.parametrize("at", [0, OUT_OFF - 1, (1 << 32) + 5, ARENA_BYTES - 1])
def test_background_check_sees_a_single_byte(cuda, arena, at):
    """The checker of (b) itself: one changed byte anywhere in the arena is found, at its offset."""
    t = arena.get()
    t[at] = POISON ^ 1
    ok, where = poison_intact(t)
    t[at] = POISON
    assert not ok and where == at // 8 * 8
    assert poison_intact(t) == (True, -1)


def test_grouped_launch_far_over(cuda, arena):
    """conv_8ph_kernel.h: with out_batch_stride given, a grouped launch keeps the caller's obs for every segment."""
    from object_detector_amd import _lib
    B, dims, Cin, Cout, act, out_f32, cfg = GROUPED_CASE
    t = arena.get()
    g, xs, rs = E.build_grouped(GROUPED_CASE)
    keep = [E._packed(g.w, g.scale, g.bias, cuda)] + [L.poisoned(x, cuda) for x in xs]
    regs = grouped_regions()
    try:
        d = _lib.ConvDesc()
        d.w, d.scale, d.bias = (x.data_ptr() for x in keep[0])
        d.B, d.Cin, d.Cout, d.ksize, d.stride = B, Cin, Cout, 3, 1
        d.act, d.alpha, d.out_dtype = _lib.ACT_ENUM[act], float(E._alpha(act)), _lib.OD_DT_F32
        d.tile_cfg, d.nseg, d.splitk = cfg, len(dims), 1
        d.out_batch_stride = GROUPED_OBS
        for i, (x, reg, (h, w)) in enumerate(zip(keep[1:], regs, dims)):
            d.seg_x[i], d.seg_out[i], d.seg_H[i], d.seg_W[i] = x.data_ptr(), t.data_ptr() + reg[0], h, w
        assert not off32(B, GROUPED_OBS, Cout, max(h * w for h, w in dims), Cout)
        name = V.run_plan(cuda, d, keep)
        got = [read_rows(t, reg, torch.float32) for reg in regs]
        check_background(arena, regs, f"{name} grouped")
        for i, (o, r) in enumerate(zip(got, rs)):
            L.assert_matches32(o.reshape(r.ref32.shape), r, f"{name} segment {i}")
        V.check_name(name, *V.expected_name((B, 0, 0, Cin, Cout, 3, 1, act, "none", cfg), out_f32=True, off32=False))
    finally:
        del keep
        torch.cuda.empty_cache()


# ---- section 2: dense [B, P, C] tensors past 2^31 elements ---------------------------------------------------------------------
P320 = 16800                  # the prior count of the 320 x 320 table (oracle.postprocess.make_priors; asserted where it is used)
PER_SPOT = 96                 # live rows per spot
# name: (NC, B, P).  Elements B * P * (NC + 6) and the image that holds element 2^31:
DENSE_SHAPES = {
    "loss74": (74, 1600, P320),          # 2 150 400 000; the widest row od_loss_rows keeps in LDS
    "wide": (1024, 125, P320),           # 2 163 000 000; 125 = the smallest batch whose LAST image holds element 2^31
    "wide126": (1024, 126, P320),        # one image more: the image with element 2^31 (124) is not the last one
    "narrow": (20, 66, 1290562),         # 2 214 604 392; image 63 holds element 2^31; P * NC < 2^31, B <= 65535
}


def sparse_rows(R, C, first_span, past_lo, seed, per=PER_SPOT):
    """The live rows of a [R, C] tensor, by spot -> sorted flat row indices: in the first image, in the 256-row block that
    holds element 2^31 and the blocks on either side, well past it, and in the last 300 rows."""
    rng = np.random.default_rng(seed)
    r31 = LIM31 // C  # the row that holds element 2^31
    blk = r31 // 256

    def pick(lo, hi, must=()):
        s = set((lo + rng.choice(hi - lo, min(per, hi - lo), replace=False)).tolist()) | set(must)
        return np.array(sorted(s), np.int64)
    return {"first": pick(0, first_span, (0,)),
            "before": pick((blk - 1) * 256, blk * 256),
            "block": pick(blk * 256, (blk + 1) * 256, (r31, blk * 256, blk * 256 + 255)),
            "after": pick((blk + 1) * 256, (blk + 2) * 256),
            "past": pick(past_lo, past_lo + 4096),
            "last": pick(R - 300, R, (R - 1,))}


def dense_layout(name, seed=0):
    """-> (NC, B, P, spots) of a DENSE_SHAPES entry: `past` lies in the last image, behind the blocks around element 2^31."""
    NC, B, P = DENSE_SHAPES[name]
    past_lo = max((B - 1) * P + 64, (LIM31 // (NC + 6) // 256 + 3) * 256)
    assert past_lo + 4096 <= B * P - 300
    return NC, B, P, sparse_rows(B * P, NC + 6, P, past_lo, seed)


def all_rows(spots):
    return np.unique(np.concatenate(list(spots.values())))


def _free(*_):
    torch.cuda.empty_cache()


def _chunks(t, n=1 << 28):
    """Views of at most n elements over the flat contiguous tensor t."""
    f = t.view(-1)
    return (f[i:i + n] for i in range(0, f.numel(), n))


def _rows_to(t2d, rows, values):
    t2d[torch.from_numpy(rows).to(t2d.device)] = torch.from_numpy(np.ascontiguousarray(values)).to(t2d.device)


def _rows_from(t2d, rows):
    return t2d[torch.from_numpy(rows).to(t2d.device)].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- loss
def loss_live_rows(NC, rows, priors, seed, iou):
    """pred / y of the live rows (numpy f32 [n, C]): half assigned (one-hot class, offsets), the rest background, every tenth
    an ignore row (all-zero target: dead for the loss, whatever pred holds).  iou: assigned rows whose decision margins
    (tests/iou_loss_ref.py) come closer than MARGIN_MIN to a min / max tie are turned into background rows."""
    import iou_loss_ref as IR
    rng = np.random.default_rng(seed)
    n, Cc = len(rows), NC + 6
    y = np.zeros((n, Cc), np.float32)
    kind = rng.integers(0, 10, n)  # 0: ignore, 1..5: assigned, 6..9: background
    pos = (kind >= 1) & (kind <= 5)
    y_loc = rng.normal(0, 1, (n, 4)).astype(np.float32)
    p_loc = (y_loc + rng.normal(0, 1.5, (n, 4))).astype(np.float32)
    if iou:
        m = IR.margins(p_loc, y_loc, priors[rows % len(priors)], IR.LOC_SCALE)
        pos &= (np.abs(m) >= IR.MARGIN_MIN).all(1)
    neg = (kind != 0) & ~pos
    y[neg, 0] = 1
    y[pos, 1] = 1
    y[np.nonzero(pos)[0], 2 + rng.integers(0, NC, int(pos.sum()))] = 1
    y[pos, -4:] = y_loc[pos]
    pred = rng.normal(0, 1.5, (n, Cc)).astype(np.float32)
    pred[:, 2:2 + NC] += 4 * y[:, 2:2 + NC]
    pred[pos, -4:] = p_loc[pos]
    assert pos.sum() >= n // 4 and neg.sum() >= n // 4
    return pred, y


def _loss_abi(cuda, entry, pred, y, priors, grad, B, P, NC, mode):
    """The C ABI with the caller's (pre-filled) grad; the workspace size as ops.loss_fwd_bwd computes it."""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    from object_detector_amd.ops import BOX_MODES
    import iou_loss_ref as IR
    ctx = Context.get(cuda)
    wsb = ctx.lib.od_loss_workspace_bytes(B, P)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=cuda)
    losses = torch.full((4,), float("nan"), dtype=torch.float32, device=cuda)
    tail = (1.0, 1.0, 1.0, ws.data_ptr(), wsb, _stream_ptr())
    if entry == "od_loss_fwd_bwd":
        rc = ctx.lib.od_loss_fwd_bwd(ctx.handle, pred.data_ptr(), y.data_ptr(), grad.data_ptr(), losses.data_ptr(), B, P, NC,
                                     0.25, 2.0, BOX_MODES[mode], *tail)
    else:
        rc = ctx.lib.od_loss_fwd_bwd_iou(ctx.handle, pred.data_ptr(), y.data_ptr(), priors.data_ptr(), grad.data_ptr(),
                                         losses.data_ptr(), B, P, NC, 0.25, 2.0, BOX_MODES[mode], IR.LOC_SCALE, *tail)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    return losses.cpu().numpy()


@pytest.mark.parametrize("entry,mode", [("od_loss_fwd_bwd", "smooth_l1"), ("od_loss_fwd_bwd_iou", "giou")])
@pytest.mark.parametrize("shape", ["loss74", "wide"])
def test_loss_past_2_31_elements(cuda, arena, shape, entry, mode):
    """pred, y, grad [B, P, NC + 6] of 8.0 GiB each.  od_loss_fwd_bwd through the C ABI into a grad pre-filled with 7 (a row
    never written is seen); od_loss_fwd_bwd_iou through ops.loss_fwd_bwd, the wrapper the trainer uses (it allocates grad
    itself), with the prior table: row r belongs to prior r % P.  Losses and live gradient rows against the CPU oracle on
    the compacted live rows (tolerances of test_loss_matches_oracle; giou box columns per row as in test_gpu_iou_loss.py,
    with the bound measured on the f32 restatement of the same rows); the giou gradient rows also bit for bit against the
    same kernel run on the compacted rows alone; grad exactly zero on every other row."""
    import iou_loss_ref as IR
    from object_detector_amd import ops
    from oracle import loss as oloss
    from oracle import postprocess as opp
    arena.free()
    NC, B, P, spots = dense_layout(shape, seed=3)
    Cc, R = NC + 6, B * P
    assert R * Cc > LIM31 and ((R - 1) * Cc > LIM31)
    need_free(cuda, 3 * R * Cc * 4 + GiB, f"loss {shape}")
    iou = mode != "smooth_l1"
    priors = opp.make_priors((320, 320))
    assert len(priors) == P320 == P
    rows = all_rows(spots)
    pl, yl = loss_live_rows(NC, rows, priors, 11, iou)
    pr_live = priors[rows % P]
    if iou:
        rl, rg = IR.full_reference(pl, yl, pr_live, NC, mode, IR.LOC_SCALE)  # row i of the compacted rows <-> prior i
    else:
        rl, rg = oloss.loss_and_grad(pl[None], yl[None], NC, box_mode=mode)
        rg = rg[0]
    assert np.isfinite(rl).all() and np.isfinite(rg).all() and (rl[:3] != 0).all()
    pred = y = grad = None
    try:
        pred = torch.empty((B, P, Cc), dtype=torch.float32, device=cuda)
        for c in _chunks(pred):  # dead rows: an all-zero target, so whatever pred holds must not matter
            c.normal_(0.0, 3.0)
        y = torch.zeros((B, P, Cc), dtype=torch.float32, device=cuda)
        _rows_to(pred.view(R, Cc), rows, pl)
        _rows_to(y.view(R, Cc), rows, yl)
        pd = torch.from_numpy(priors).to(cuda)
        if iou:
            losses, grad = ops.loss_fwd_bwd(pred, y, NC, box_mode=mode, priors=pd, loc_scale=IR.LOC_SCALE)
            torch.cuda.synchronize()
            losses = losses.cpu().numpy()
        else:
            grad = torch.full((B, P, Cc), 7.0, dtype=torch.float32, device=cuda)
            losses = _loss_abi(cuda, entry, pred, y, None, grad, B, P, NC, mode)
        g2 = grad.view(R, Cc)
        gl = _rows_from(g2, rows)
        print(f"loss {shape} {mode}: losses {losses}, reference {rl}")
        assert np.isfinite(losses).all() and np.isfinite(gl).all()
        np.testing.assert_allclose(losses, rl, rtol=2e-5)
        if iou:
            np.testing.assert_allclose(gl[:, :-4], rg[:, :-4], rtol=1e-4, atol=1e-8)
            pos = yl[:, 1] > 0.5
            _l, g64 = IR.loss_and_grad(pl[pos, -4:], yl[pos, -4:], pr_live[pos], IR.LOC_SCALE, mode)
            _l, g32 = IR.loss_and_grad_f32(pl[pos, -4:], yl[pos, -4:], pr_live[pos], IR.LOC_SCALE, mode)
            bound = 4 * float(IR.row_rel_err(g32, g64).max())  # test_gpu_iou_loss.py: 4 x the f32 restatement's own error
            err = IR.row_rel_err(gl[pos, -4:], rg[pos, -4:])
            print(f"loss {shape} {mode}: worst row-relative box-gradient error {err.max():.3e}, bound {bound:.3e}")
            assert (gl[~pos, -4:] == 0).all() and (err <= bound).all()
            # the same kernel on the compacted rows alone (B = 1, P = n, prior i for row i): the same bits row by row
            small = torch.full((len(rows), Cc), 7.0, dtype=torch.float32, device=cuda)
            _loss_abi(cuda, entry, torch.from_numpy(pl).to(cuda), torch.from_numpy(yl).to(cuda),
                      torch.from_numpy(np.ascontiguousarray(pr_live)).to(cuda), small, 1, len(rows), NC, mode)
            assert np.array_equal(small.cpu().numpy().view(np.int32), gl.view(np.int32))
        else:
            np.testing.assert_allclose(gl, rg, rtol=1e-4, atol=1e-8)
        # every other row: exactly zero (the live rows are cleared first; chunked count on the device)
        g2[torch.from_numpy(rows).to(cuda)] = 0
        nz = sum(int(torch.count_nonzero(c)) for c in _chunks(grad))
        assert nz == 0, f"{nz} non-zero gradient elements on rows whose target is all zero"
    finally:
        del pred, y, grad
        _free()


# ---------------------------------------------------------------------------------------------- detection: head, top-K, od_detect
IOU_THR, CONF_THR, TOPK, MAX_DET = 0.45, 0.05, 1024, 200
DEAD_ROW = (20.0, -20.0, -12.0, 0.0)  # test_gpu_detect_tail.py::_case: objectness e^-40, class logits -12, zero offsets


def detect_priors(P, seed):
    """The real 320 x 320 table where P is its size, random well-formed boxes otherwise (test_gpu_detect_tail.py)."""
    from oracle import postprocess as opp
    if P == P320:
        return opp.make_priors((320, 320))
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0.1, 0.9, (P, 2)).astype(np.float32)
    wh = rng.uniform(0.05, 0.3, (P, 2)).astype(np.float32)
    return np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)


def detect_live_rows(NC, spots, seed):
    """-> (rows, pred rows f32 [n, C]).  The rows of the blocks around element 2^31 hold random logits with a favourable
    objectness (several scores per row above the threshold: more than K candidates in that image, so the candidate list at
    image * cand_stride is written and refined); every other live row has exactly one score above it (_hot)."""
    rng = np.random.default_rng(seed)
    rows = all_rows(spots)
    n, Cc = len(rows), NC + 6
    pred = np.empty((n, Cc), np.float32)
    pred[:, 0], pred[:, 1], pred[:, 2:2 + NC], pred[:, 2 + NC:] = DEAD_ROW
    d = rng.uniform(2, 6, n).astype(np.float32)
    pred[:, 0], pred[:, 1] = -d / 2, d / 2
    pred[:, 2 + NC:] = rng.normal(0, 1, (n, 4))
    busy = np.isin(rows, np.concatenate([spots["before"], spots["block"], spots["after"]]))
    pred[np.nonzero(~busy)[0], 2 + rng.integers(0, NC, int((~busy).sum()))] = 12.0
    nb = int(busy.sum())
    logits = np.full((nb, NC), -12.0, np.float32)
    for i in range(nb):  # up to 8 classes share the row's probability: each score 0.1 .. 0.9 of the objectness
        cls = rng.choice(NC, min(NC, 8), replace=False)
        logits[i, cls] = rng.normal(0, 1.5, len(cls))
    pred[busy, 2:2 + NC] = logits
    return rows, pred


def _dense_pred(cuda, B, P, NC, rows, live):
    pred = torch.empty((B * P, NC + 6), dtype=torch.float32, device=cuda)
    row = np.empty(NC + 6, np.float32)
    row[0], row[1], row[2:2 + NC], row[2 + NC:] = DEAD_ROW
    pred[:] = torch.from_numpy(row).to(cuda)
    _rows_to(pred, rows, live)
    return pred.view(B, P, NC + 6)


def _compact_head(cuda, live, pr_live, NC):
    """od_head_postprocess on the live rows alone (B = 1, P = n, prior i for row i): the device's confidences of those rows,
    bit for bit what every kernel that calls od_row_conf / od_wide_conf computes for them."""
    from object_detector_amd.postprocess import Postprocessor
    pp = Postprocessor(1, len(live), NC, pr_live, device=cuda, topk=TOPK, max_det=MAX_DET)
    conf, boxes = pp.head(torch.from_numpy(live[None]).to(cuda))
    torch.cuda.synchronize()
    return conf[0].cpu().numpy(), boxes[0].cpu().numpy()


def _image_tables(rows, conf_live, boxes_live, b, P, NC):
    """The confidence and box tables of image b with every dead row at zero: -> (conf f32 [P * NC], boxes f32 [P, 4])."""
    sel = rows // P == b
    p = rows[sel] - b * P
    conf = np.zeros((P, NC), np.float32)
    boxes = np.zeros((P, 4), np.float32)
    conf[p], boxes[p] = conf_live[sel], boxes_live[sel]
    return conf.reshape(-1), boxes


def test_head_and_topk_past_2_31_elements(cuda, arena):
    """od_head_postprocess at NC = 1024, B = 126: pred AND conf pass 2^31 elements; then od_topk_scores on that conf."""
    from object_detector_amd.postprocess import Postprocessor
    from oracle import nms as onms
    from oracle import postprocess as opp
    arena.free()
    NC, B, P, spots = dense_layout("wide126", seed=5)
    R, Cc = B * P, NC + 6
    assert R * NC > LIM31
    need_free(cuda, R * Cc * 4 + 2 * R * NC * 4 + GiB, "head + top-K, NC = 1024")
    priors = detect_priors(P, 1)
    rows, live = detect_live_rows(NC, spots, 21)
    pred = pp = None
    try:
        pred = _dense_pred(cuda, B, P, NC, rows, live)
        pp = Postprocessor(B, P, NC, priors, device=cuda, topk=TOPK, max_det=MAX_DET, iou_threshold=IOU_THR)
        conf, boxes = pp.head(pred)
        torch.cuda.synchronize()
        assert conf.numel() > LIM31
        # live rows, and 300 sampled dead rows, against the CPU oracle: boxes bit-exact, conf as in test_head_postprocess
        dead = np.setdiff1d(np.random.default_rng(2).choice(R, 300, replace=False), rows)
        check = np.concatenate([rows, dead])
        pc = _rows_from(pred.view(R, Cc), check)
        rconf, rboxes = opp.head_postprocess(pc[None], priors[check % P], NC)
        gconf, gboxes = _rows_from(conf.view(R, NC), check), _rows_from(boxes.view(R, 4), check)
        assert np.array_equal(gboxes, rboxes[0])
        np.testing.assert_allclose(gconf, rconf[0], rtol=2e-6, atol=1e-7)
        # every dead row holds the same prediction, hence the same confidences bit for bit: on the device, image by image
        dead_conf = conf.view(R, NC)[int(dead[0])].clone()
        live_mask = torch.zeros(R, dtype=torch.bool, device=cuda)
        live_mask[torch.from_numpy(rows).to(cuda)] = True
        bad = sum(int((~((conf[b] == dead_conf).all(1) | live_mask[b * P:(b + 1) * P])).sum()) for b in range(B))
        assert bad == 0, f"{bad} dead rows whose confidences differ from the dead row's"
        keys, counts = pp.topk(conf, CONF_THR)
        torch.cuda.synchronize()
        counts, keys = counts.cpu().numpy(), keys.cpu().numpy().view(np.uint64)
        b31 = LIM31 // NC // P  # conf's own element 2^31
        imgs = sorted({0, b31, LIM31 // Cc // P, B - 1})
        assert len(imgs) >= 3
        for b in imgs:
            ref = onms.topk_keys(conf[b].reshape(-1).cpu().numpy(), TOPK, CONF_THR)
            assert counts[b] == len(ref) > 0, (b, counts[b], len(ref))
            got = np.sort(keys[b][keys[b] != 0])[::-1]
            assert np.array_equal(got, ref), f"image {b}"
        live_imgs = np.unique(rows // P)
        assert (np.delete(counts, live_imgs) == 0).all()
    finally:
        del pred, pp
        conf = boxes = dead_conf = live_mask = None
        _free()


@pytest.mark.parametrize("shape", ["narrow", "wide126"])
def test_detect_past_2_31_elements(cuda, arena, shape):
    """od_detect, then od_gather_detections_pred, through Postprocessor.run / .gather: keys, counts, kept indices and the
    record block of every image that has live rows against oracle/nms.py fed the device's confidences and boxes of the live
    rows, exactly; every other image empty.  narrow: NC = 20 (compile-time pass 1, the candidate list of image 63 lies 13 GB
    into the workspace); wide126: the streamed kernels of detect_wide.hip."""
    from object_detector_amd.postprocess import Postprocessor
    from oracle import nms as onms
    from oracle import postprocess as opp
    arena.free()
    NC, B, P, spots = dense_layout(shape, seed=7)
    R, Cc = B * P, NC + 6
    priors = detect_priors(P, 3)
    rows, live = detect_live_rows(NC, spots, 23)
    pred = pp = None
    try:
        lib = __import__("object_detector_amd._lib", fromlist=["load"]).load()
        need = R * Cc * 4 + lib.od_detect_workspace_bytes(B, P, NC, TOPK) + R * 16 + GiB
        assert need < 27 * GiB
        need_free(cuda, need, f"od_detect {shape}")
        pred = _dense_pred(cuda, B, P, NC, rows, live)
        pp = Postprocessor(B, P, NC, priors, device=cuda, topk=TOPK, max_det=MAX_DET, iou_threshold=IOU_THR)
        assert pp.fused
        pp.keys.fill_(-1), pp.counts.fill_(-7), pp.keep_flat.fill_(-9), pp.keep_count.fill_(-9), pp.boxes.fill_(7.0)
        kf, kc = pp.run(pred, CONF_THR)
        pp.gather()
        torch.cuda.synchronize()
        conf_live, boxes_small = _compact_head(cuda, live, priors[rows % P], NC)
        boxes_live = _rows_from(pp.boxes.view(R, 4), rows)
        assert np.array_equal(boxes_live, boxes_small)
        assert np.array_equal(boxes_live, opp.head_postprocess(live[None], priors[rows % P], NC)[1][0])  # bit-exact decode
        counts, kcount = pp.counts.cpu().numpy(), kc.cpu().numpy()
        keys, keep = pp.keys.cpu().numpy().view(np.uint64), kf.cpu().numpy()
        det = pp.detections_host(B)
        live_imgs = np.unique(rows // P)
        b31 = LIM31 // Cc // P
        assert {0, b31, B - 1} <= set(live_imgs.tolist())
        for b in live_imgs:
            cflat, bx = _image_tables(rows, conf_live, boxes_live, b, P, NC)
            ref = onms.topk_keys(cflat, TOPK, CONF_THR)
            n = len(ref)
            assert counts[b] == n > 0, (b, counts[b], n)
            assert np.array_equal(keys[b, :n], ref) and (keys[b, n:] == 0).all(), f"keys of image {b}"
            rk = onms.nms_image(bx, ref, NC, IOU_THR, False, MAX_DET)
            assert kcount[b] == len(rk) > 0 and np.array_equal(keep[b, :len(rk)], rk) and (keep[b, len(rk):] == -1).all(), b
            flat, dconf, dbox = det[b]
            assert np.array_equal(flat, rk) and np.array_equal(dconf, cflat[rk]) and np.array_equal(dbox, bx[rk // NC]), b
        assert counts[b31] == TOPK, "the image around element 2^31 must overflow K (the candidate-list path)"
        others = np.delete(np.arange(B), live_imgs)
        assert (counts[others] == 0).all() and (kcount[others] == 0).all() and (keep[others] == -1).all()
    finally:
        del pred, pp
        kf = kc = None
        _free()


# ---------------------------------------------------------------------------------------------------------- assignment
def _annotations(B, ignore):
    """GT of the batch: images 0, 1, B - 2 and B - 1 get boxes of their own (image 1's are those of every remaining image).
    ignore: some boxes are flagged as ignore regions (`difficults`)."""
    from object_detector_amd.pb import ObjectsAnnotation

    def ann(seed, n):
        rng = np.random.default_rng(seed)
        c = rng.uniform(0.15, 0.85, (n, 2))
        wh = rng.uniform(0.05, 0.5, (n, 2))
        b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)
        cls = rng.integers(0, 1024, n)
        cls[0] = 1023
        flags = rng.integers(0, 3, n) == 0
        flags[0], flags[-1] = False, True  # at least one box that owns priors, at least one region
        return ObjectsAnnotation(None, 320, 320, cls, b, flags if ignore else None)
    own = {0: ann(100, 7), B - 2: ann(101, 12), B - 1: ann(102, 5)}
    common = ann(103, 3)
    return [own.get(b, common) for b in range(B)]


@pytest.mark.parametrize("entry", ["od_assign_anchors", "od_assign_anchors_ign", "od_assign_atss", "od_assign_tal"])
def test_assign_past_2_31_elements(cuda, arena, entry):
    """PriorBoxes.encode_batch(return_device=True) at NC = 1024, P = 16800, B = 125: y of 8.06 GiB; y, assigned_gt and npos of
    images 0, 1, 123 and 124 against the assigner's reference (oracle/assign.py, tests/assign_ign_ref.py, tests/atss_ref.py:
    bit for bit; tests/tal_ref.py: its parity rule, check_image), every other image against image 1's rows on the device.
    od_assign_atss and od_assign_tal write y in od_claim_encode, a kernel of their own, and od_assign_tal reads pred
    (8.06 GiB more, images 2 .. 122 copies of image 1) in od_tal_prior / od_tal_claims.  encode_batch allocates y itself: a
    NaN-filled tensor of the same size is freed right before the call, so that the allocator hands the kernel that block and
    a row it does not write stays NaN."""
    import assign_ign_ref as AR
    import atss_ref
    import tal_ref
    from object_detector_amd import priors as PR
    from object_detector_amd.pb import PriorBoxes
    from oracle import assign as oassign
    arena.free()
    NC, B, P = DENSE_SHAPES["wide"]
    Cc = NC + 6
    assert (B - 1) * P * Cc <= LIM31 < B * P * Cc, "125 must be the smallest batch whose last image holds element 2^31"
    tal, ignore = entry == "od_assign_tal", entry == "od_assign_anchors_ign"
    need_free(cuda, (3 if tal else 2) * B * P * Cc * 4 + GiB, f"{entry}, NC = 1024")
    pb = PriorBoxes((320, 320), NC, device=cuda, ignore_regions=ignore,
                    assigner={"od_assign_atss": "atss", "od_assign_tal": "tal"}.get(entry, "max-iou"))
    assert len(pb) == P
    levels = PR.level_shapes((320, 320))
    anns = _annotations(B, ignore)
    y = ref = pred = None
    try:
        if tal:
            pred = torch.empty((B, P, Cc), dtype=torch.float32, device=cuda)
            for b in (0, 1, B - 2, B - 1):
                pred[b].normal_(0.0, 1.5)
            pred[2:B - 2] = pred[1]
        poison = torch.full((B, P, Cc), float("nan"), dtype=torch.float32, device=cuda)
        del poison
        y, npos, assigned = pb.encode_batch(anns, return_device=True, pred=pred)
        torch.cuda.synchronize()
        assert y.numel() > LIM31
        npos_h = npos.cpu().numpy()
        for b in (0, 1, B - 2, B - 1):
            a = anns[b]
            if tal:
                r = tal_ref.encode_truth(a.bboxes, a.classes, pred[b].cpu().numpy(), pb.pb_locs, levels, NC, topk=pb.tal_topk,
                                         alpha=pb.tal_alpha, beta=pb.tal_beta, loc_scale=pb.loc_scale)
                worst = tal_ref.check_image(r, a.bboxes, a.classes, pb.pb_locs, NC, y[b].cpu().numpy(), assigned[b].cpu().numpy(),
                                            int(npos_h[b]), pb.last_metric[b].cpu().numpy(), loc_scale=pb.loc_scale)
                print(f"od_assign_tal image {b}: max |metric - l| / (1 + |l|) = {worst:.3g}, npos {npos_h[b]}")
                assert npos_h[b] > 0
                continue
            if ignore:
                ry, ra = AR.encode_truth(a.bboxes, a.classes, pb.pb_locs, NC, flags=a.difficults.astype(np.int32), ign_thr=pb.ign_thr)
            elif entry == "od_assign_atss":
                ry, ra = atss_ref.encode_truth(a.bboxes, a.classes, pb.pb_locs, levels, NC, topk=pb.atss_topk)
            else:
                ry, ra = oassign.encode_truth(a.bboxes, a.classes, pb.pb_locs, NC)
            ref = torch.from_numpy(ry).to(cuda)
            assert torch.equal(y[b], ref), f"y of image {b}"
            assert np.array_equal(assigned[b].cpu().numpy(), ra), f"assigned_gt of image {b}"
            assert npos_h[b] == int((ra >= 0).sum()) > 0, b
        for b in range(2, B - 2):  # image 1's rows have just been checked against the reference
            assert torch.equal(y[b], y[1]) and torch.equal(assigned[b], assigned[1]) and npos_h[b] == npos_h[1], b
            assert not tal or torch.equal(pb.last_metric[b], pb.last_metric[1]), b
    finally:
        del y, ref, pred
        pb.last_metric = None
        _free()


# ------------------------------------------------------------------------------------------------- od_pred_grad_to_level
@pytest.mark.parametrize("scale", [1024.0])
def test_pred_grad_to_level_past_2_31_elements(cuda, arena, scale):
    """grad_pred [125, 16800, 1030] f32: the last level's rows (the last 600 of every image) -> loss-scaled f16.  The slice of
    the last image lies wholly past element 2^31.  Images 0, 123 and 124 bit for bit against numpy's round-to-nearest-even
    conversion (the restatement of tests/test_gpu_loss.py), every image against torch's conversion on the device."""
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    arena.free()
    NC, B, P = DENSE_SHAPES["wide"]
    Cc, rows = NC + 6, 600
    row_off = P - rows
    assert ((B - 1) * P + row_off) * Cc > LIM31
    need_free(cuda, B * P * Cc * 4 + 2 * GiB, "od_pred_grad_to_level")
    ctx = Context.get(cuda)
    g = dz = want = None
    try:
        g = torch.empty((B, P, Cc), dtype=torch.float32, device=cuda)
        for c in _chunks(g):
            c.normal_(0.0, 1.0)
        sl = g[:, row_off:]
        sl.mul_(torch.exp2(torch.randint(-30, 8, sl.shape, device=cuda).float()))  # down to f16 denormals, up to overflow
        G = 64
        n = B * rows * Cc
        dz = torch.full((n + 2 * G,), 0x5A5A, dtype=torch.int16, device=cuda)
        _lib.check(ctx.lib.od_pred_grad_to_level(ctx.handle, g.data_ptr(), dz.data_ptr() + 2 * G, B, P, Cc, row_off, rows, scale,
                                                 _stream_ptr()), "od_pred_grad_to_level")
        torch.cuda.synchronize()
        assert bool((dz[:G] == 0x5A5A).all()) and bool((dz[G + n:] == 0x5A5A).all()), "guard elements around dz written"
        got = dz[G:G + n].view(B, rows, Cc)
        want = (sl * scale).to(torch.float16).view(torch.int16)
        assert torch.equal(got, want)
        for b in (0, B - 2, B - 1):
            src = sl[b].cpu().numpy()
            with np.errstate(over="ignore"):
                ref = (src * np.float32(scale)).astype(np.float16)
            assert np.isinf(ref).sum() > 0 and (ref == 0).sum() > 0
            assert np.array_equal(got[b].cpu().numpy().view(np.uint16), ref.view(np.uint16)), f"image {b}"
    finally:
        del g, dz, want
        sl = got = None
        _free()


# ---- section 3: conv INPUTS between 2 GiB and 4 GiB ----------------------------------------------------------------------------
# x is f16 [B, H, W, 64], zero except for a few 5 x 5 patches of lattice values; the reference (lattice_ref) is computed on
# each patch's neighbourhood only, and everywhere else the output must be the epilogue of a zero sum.  tile_cfg = -1: the
# library's own choice is what is tested, through conv_choose_cfg's gate `x_bytes < 0x7F000000` on the 8-wave kernel (its
# loaders form byte offsets in 31 bits).  pick_cfg never offers the 8-wave kernel to a layer of <= 64 output channels, so the
# two cases at the gate are a 64 -> 256 layer with stride 2 (its output, 2.1 GB, stays below 2^31 elements); the case just
# below 4 GiB keeps Cout = 8.  The table kernels form ELEMENT offsets in 32 bits, good for the whole admitted range.
GATE = 0x7F000000
InCase = collections.namedtuple("InCase", "name B H W Cout k stride kernel")
IN_CASES = [InCase(f"{n}-{k}x{k}", B, H, W, cout, k, s, kern) for k in (3, 1) for n, B, H, W, cout, s, kern in (
    ("below-gate", 1, 4095, 4064, 256, 2, "od_conv_8ph<"),    # x_bytes = 0x7F000000 - 520 192 (one image row)
    ("at-gate", 1, 4096, 4064, 256, 2, "od_conv_igemm<"),     # x_bytes = 0x7F000000 exactly: the first size the gate refuses
    ("below-4GiB", 31, 601, 1801, 8, 1, "od_conv_igemm<"))]   # B * H * W * 64 = 2^31 - 64 elements, the largest admitted
IN_REFUSED = (32, 1024, 1024)  # B * H * W * 64 = 2^31: one pixel more than "below-4GiB"
PATCH, MARGIN = 5, 2           # the patch and the ring of zeros around it that the reference window includes (even: stride 2)


def input_patches(ic):
    """Top-left corners (b, y, x) of the patches of a case: at the start, in the middle (around byte 2^31 where the input
    reaches it: the patch then has pixels on both sides), at the very end (the last legal pixel is its last)."""
    B, H, W = ic.B, ic.H, ic.W
    out = [(0, 0, 0), (B - 1, H - PATCH, W - PATCH)]
    pix31 = LIM31 // 128  # the pixel whose first byte is byte 2^31
    if B * H * W > pix31:
        b, r = divmod(pix31, H * W)
        y, x = divmod(r, W)
        out.append((b, y - 2, x - 2))
        out.append((B - 1, H - PATCH - 40, 6))  # well past it, away from the corner patch
    else:
        out.append((B // 2, (H // 2) & ~1, (W // 2) & ~1))
    return out


def patch_window(ic, y, x):
    """The input window of the reference for a patch at (y, x): the patch and MARGIN pixels around it, cut at the image's
    border, its origin even -> (y0, y1, x0, x1)."""
    y0, x0 = max(0, y - MARGIN) & ~1, max(0, x - MARGIN) & ~1
    return y0, min(ic.H, y + PATCH + MARGIN), x0, min(ic.W, x + PATCH + MARGIN)


@pytest.mark.parametrize("ic", IN_CASES, ids=[c.name for c in IN_CASES])
def test_conv_input_between_2_and_4_gib(cuda, arena, ic):
    from object_detector_amd import _lib
    arena.free()
    x_bytes = ic.B * ic.H * ic.W * 64 * 2
    assert (x_bytes < GATE) == ic.kernel.startswith("od_conv_8ph") and ic.B * ic.H * ic.W * 64 < LIM31
    Ho, Wo = L.out_hw(ic.H, ic.W, ic.stride)
    assert ic.B * Ho * Wo * ic.Cout < LIM31
    need_free(cuda, x_bytes + ic.B * Ho * Wo * ic.Cout * 2 + 2 * GiB, f"conv input {ic.name}")
    g = L.gen_conv(("large-input", ic.Cout, ic.k, ic.stride), 1, 8, 8, 64, ic.Cout, ic.k, ic.stride, "none", "leaky")
    alpha = E._alpha("leaky")
    rng = np.random.default_rng(L.seed_of("large-input-patches", ic.name))
    zero = L.epilogue(np.zeros((1, 1, 1, ic.Cout)), g.scale, g.bias, "leaky", alpha).ref16.reshape(-1)  # act(bias), rounded once
    x = out = neq = None
    keep = [E._packed(g.w, g.scale, g.bias, cuda)]
    try:
        x = torch.zeros((ic.B, ic.H, ic.W, 64), dtype=torch.float16, device=cuda)
        out = torch.full((ic.B, Ho, Wo, ic.Cout), float("nan"), dtype=torch.float16, device=cuda)
        wins = []
        for b, y, xx in input_patches(ic):
            pv = rng.integers(-8, 9, (PATCH, PATCH, 64)).astype(np.float16)
            x[b, y:y + PATCH, xx:xx + PATCH] = torch.from_numpy(pv).to(cuda)
            y0, y1, x0, x1 = patch_window(ic, y, xx)
            crop = np.zeros((1, y1 - y0, x1 - x0, 64), np.float16)
            crop[0, y - y0:y - y0 + PATCH, xx - x0:xx - x0 + PATCH] = pv
            wins.append((b, y0, y1, x0, x1, L.ref_forward(crop, g.w, g.scale, g.bias, ic.stride, "leaky", alpha,
                                                          what=f"{ic.name} patch at {(b, y, xx)}", rounding=False)))
        d = _lib.ConvDesc()
        d.x, d.out = x.data_ptr(), out.data_ptr()
        d.w, d.scale, d.bias = (t.data_ptr() for t in keep[0])
        d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = ic.B, ic.H, ic.W, 64, ic.Cout, ic.k, ic.stride
        d.act, d.alpha, d.res_mode, d.out_dtype = _lib.ACT_ENUM["leaky"], float(alpha), _lib.OD_RES_NONE, _lib.OD_DT_F16
        d.tile_cfg, d.splitk = -1, 1
        name = V.run_plan(cuda, d, [])
        assert name.startswith(ic.kernel), f"{ic.name}: resolved to {name}"
        # every output pixel that differs from the zero-sum value, on the device (one bool per pixel)
        zt = torch.from_numpy(zero).to(cuda)
        neq = torch.empty((ic.B, Ho, Wo), dtype=torch.bool, device=cuda)
        for b in range(ic.B):
            for r0 in range(0, Ho, 256):
                neq[b, r0:r0 + 256] = ~(out[b, r0:r0 + 256] == zt).all(-1)
        for b, y0, y1, x0, x1, r in wins:
            oy0, ox0 = y0 // ic.stride, x0 // ic.stride
            h, w = r.ref16.shape[1:3]
            got = out[b, oy0:oy0 + h, ox0:ox0 + w].cpu().numpy()
            L.assert_matches(got[None], r, f"{name} {ic.name} window at image {b} ({y0}, {x0})")
            assert bool(neq[b, oy0:oy0 + h, ox0:ox0 + w].any()), "the patch must be visible in the output"
            neq[b, oy0:oy0 + h, ox0:ox0 + w] = False
        bad = int(neq.sum())
        assert bad == 0, f"{name} {ic.name}: {bad} output pixels outside the patches' neighbourhoods differ from act(bias)"
    finally:
        del x, out, neq, keep
        _free()


# ---- section 4: refusals (the error code, no launch; every pointer is a real allocation) -------------------------------------
def test_size_guards_refuse(cuda, arena):
    from object_detector_amd import _lib
    from object_detector_amd.net import Context, _stream_ptr
    arena.free()
    ctx = Context.get(cuda)
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
    ptr = buf.data_ptr()
    INVALID = -1  # OD_ERR_INVALID (include/odhip.h)

    def conv(B, H, W, Cin, Cout, segs=()):
        d = _lib.ConvDesc()
        d.x = d.w = d.scale = d.bias = d.out = ptr
        d.B, d.H, d.W, d.Cin, d.Cout, d.ksize, d.stride = B, H, W, Cin, Cout, 3, 1
        d.out_dtype, d.tile_cfg, d.splitk, d.nseg = _lib.OD_DT_F16, -1, 1, len(segs)
        for i, (h, w) in enumerate(segs):
            d.seg_x[i], d.seg_out[i], d.seg_H[i], d.seg_W[i] = ptr, ptr, h, w
        return ctx.lib.od_conv2d_fwd(ctx.handle, C.byref(d), _stream_ptr())
    # conv_describe (csrc/conv_dispatch.hip): `M64 * Cout < 2^31 && B * H * W * Cin < 2^31`
    assert conv(1, 4096, 4096, 8, 128) == INVALID              # output: 2^24 pixels x 128 = 2^31 elements
    assert conv(1, 4096, 4096, 128, 8) == INVALID              # input: the same the other way round
    assert conv(IN_REFUSED[0], IN_REFUSED[1], IN_REFUSED[2], 64, 8) == INVALID  # one pixel more than test_conv_input's largest
    assert b"too large" in ctx.lib.od_last_error()
    # conv_describe, grouped launch: `Mg * Cout < 2^31` over all segments (each segment alone is admitted) ...
    assert conv(1, 0, 0, 64, 256, segs=[(2048, 2048), (2048, 2048)]) == INVALID
    assert b"grouped launch too large" in ctx.lib.od_last_error()
    # ... and the input extent of EVERY segment, not only of the first
    assert conv(1, 0, 0, 1024, 8, segs=[(16, 16), (2048, 1024)]) == INVALID
    assert b"grouped launch too large" in ctx.lib.od_last_error()
    # od_detect (csrc/detect.hip, det_run): `(long long)P * NC < 2^31`
    rc = ctx.lib.od_detect(ctx.handle, ptr, ptr, 1, 1 << 21, 1024, 0.1, 1, 0.05, 1024, 0.45, 0, 200, ptr, None, ptr, ptr, ptr,
                           ptr, ptr, 1 << 40, ptr, 1 << 40, _stream_ptr())
    assert rc == INVALID and b"P * NC must fit 31 bits" in ctx.lib.od_last_error()
    # od_assign_tal (csrc/assign_tal.hip): `blocks <= 0x7FFFFFFF`, "B * P too large": 4 rows per block at NC = 1024
    grid = (C.c_int32 * 2)(512, 512)
    rc = ctx.lib.od_assign_tal(ctx.handle, ptr, grid, 1, 1, ptr, ptr, ptr, ptr, None, 0.5, 1.0, 6.0, 13, 32768, 512 * 512, 4, 1024,
                               0.1, ptr, ptr, ptr, ptr, ptr, 1 << 40, _stream_ptr())
    assert rc == INVALID and b"B * P too large" in ctx.lib.od_last_error()
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0, "a refused call wrote to the buffer"
