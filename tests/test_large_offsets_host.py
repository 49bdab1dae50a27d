"""CPU halves of tests/test_gpu_large_offsets.py: which side of conv_describe's `off32` predicate (csrc/conv_dispatch.hip),
or of conv_choose_cfg's 0x7F000000 gate, every conv case is on; that everything a case writes lies inside the arena and that
no two rows of a case overlap; and that the sparse layouts of the dense tensors have live rows on both sides of element
2^31, in the 256-row block that holds it, and in the tensor's last rows -- all without a GPU."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import test_gpu_large_offsets as T  # noqa: E402

LIM31 = 1 << 31


def _check_regions(regions, what):
    spans = []
    for reg in regions:
        byte0, B, hw, Cout, obs, ops, es = reg
        assert byte0 % 16 == 0 and obs % T.ALIGN == 0 and ops % T.ALIGN == 0, f"{what}: a 16-byte store would be misaligned"
        starts = np.sort(T.row_starts(reg))
        assert starts[0] >= 0 and (np.diff(starts) >= Cout).all(), f"{what}: two written rows overlap"
        lo, hi = byte0 + int(starts[0]) * es, byte0 + (int(starts[-1]) + Cout) * es
        assert T.OUT_OFF <= lo and hi <= T.ARENA_BYTES, f"{what}: bytes [{lo}, {hi}) leave the arena"
        spans.append((lo, hi, starts * es + byte0, Cout * es))
    # rows of different regions (the segments of the grouped launch) do not overlap either
    allrows = np.sort(np.concatenate([s[2] for s in spans]))
    width = max(s[3] for s in spans)
    assert (np.diff(allrows) >= width).all() or len(spans) == 1, f"{what}: regions overlap"


@pytest.mark.parametrize("oc", T.OUT_CASES, ids=[c.name for c in T.OUT_CASES])
def test_conv_output_case_sits_where_its_name_says(oc):
    B, H, W, _cin, Cout = oc.layer[:5]
    assert T.off32(B, oc.obs, oc.ops, H * W, Cout) == oc.off32
    last = T.last_offset(oc.layer, oc.obs, oc.ops)
    if oc.name.startswith("last-under"):
        assert last == LIM31 - 1 - T.ALIGN and B * oc.obs < LIM31
    elif oc.name.startswith("last-over"):
        assert last == LIM31 - 1 and B * oc.obs < LIM31
    elif oc.name.startswith("bobs-under"):
        assert B * oc.obs < LIM31 <= B * (oc.obs + T.ALIGN) and last < LIM31 - 1
    elif oc.name.startswith("bobs-over"):
        assert B * oc.obs >= LIM31 and last < LIM31 - 1 and B * (oc.obs - T.ALIGN) < LIM31
    elif oc.name.startswith(("far", "splitk")):
        assert (B - 1) * oc.obs >= LIM31, "the last image must start past 2^31 elements"
    elif oc.name.startswith("pix-ops2^25"):
        assert (H * W - 1) * oc.ops >= LIM31 and B * oc.obs < LIM31, "pixel * ops alone must pass 2^31"
    _check_regions(T.regions_of(oc), oc.name)


def test_far_cases_reach_past_2_32_on_the_f16_view():
    far = [c for c in T.FAR_CASES if not c.out_f32 and c.obs == (1 << 31) + 8]
    assert len(far) == 4 and all((c.layer[0] - 1) * c.obs >= 1 << 32 for c in far)
    assert len(T.FAR_CASES) == 12 and sum(c.out_f32 for c in T.FAR_CASES) == 4
    # a table config 1x1 and 3x3 and an 8-wave tile height 3x3 and 1x1, on each view and stride
    for is32 in (False, True):
        kinds = {(c.layer[9] >= T.NE8, c.layer[5]) for c in T.FAR_CASES if c.out_f32 == is32}
        assert kinds == {(False, 1), (False, 3), (True, 1), (True, 3)}


def test_boundary_pairs_share_their_reference():
    """'The bits must be the same as in the case under the boundary': both cases of a pair are compared with ONE reference
    tensor (build_fwd caches by layer), so equality with it on both sides is equality with each other."""
    cases = T.BOUNDARY_CASES
    assert len(cases) == 4 * len(T.BOUNDARY_LAYERS)
    for a, b in zip(cases[0::2], cases[1::2]):
        assert a.layer == b.layer and a.out_f32 == b.out_f32 and a.off32 and not b.off32
        assert T.E.build_fwd(a.layer, out_f32=a.out_f32)[1] is T.E.build_fwd(b.layer, out_f32=b.out_f32)[1]


def test_expected_names_on_either_side():
    V = T.V
    assert V.expected_name(T.F32_E8[0], out_f32=True)[0] == "od_conv_8ph<3, 4, 16, -1, false, true>"
    assert V.expected_name(T.F32_E8[0], out_f32=True, off32=False)[0] == "od_conv_8ph<3, 4, -1, -1, false, true>"
    for layer, f32 in T.BOUNDARY_LAYERS:
        under, over = V.expected_name(layer, out_f32=f32)[0], V.expected_name(layer, out_f32=f32, off32=False)[0]
        assert "-1>" not in under and ", -1, -1," not in under, under  # a compiled policy
        assert over.endswith("-1>") or ", -1, -1," in over, over
    # the default leaves the existing cases as they were
    assert V.expected_name(V.E8_F16_CASES[0]) == V.expected_name(V.E8_F16_CASES[0], off32=True)


def test_grouped_case():
    B, dims, _cin, Cout = T.GROUPED_CASE[:4]
    assert T.GROUPED_CASE[5] is True and (B - 1) * T.GROUPED_OBS >= LIM31
    assert not T.off32(B, T.GROUPED_OBS, Cout, max(h * w for h, w in dims), Cout)
    _check_regions(T.grouped_regions(), "grouped")
    g, xs, rs = T.E.build_grouped(T.GROUPED_CASE)
    assert all(r.ref32.dtype == np.float32 and np.isfinite(r.ref32).all() for r in rs)


@pytest.mark.parametrize("name", sorted(T.DENSE_SHAPES))
def test_sparse_layouts(name):
    NC, B, P, spots = T.dense_layout(name)
    C, R = NC + 6, B * P
    assert R * C > LIM31 and B <= 65535 and P * NC < LIM31 and P % 2 == 0
    r31 = LIM31 // C
    assert r31 * C <= LIM31 < (r31 + 1) * C
    rows = T.all_rows(spots)
    assert rows[0] == 0 and rows[-1] == R - 1 and len(np.unique(rows)) == len(rows) and len(rows) < 4000
    assert (spots["first"] < P).all(), "no live row in image 0"
    blk = r31 // 256
    for spot, k in (("before", blk - 1), ("block", blk), ("after", blk + 1)):
        assert (spots[spot] // 256 == k).all() and len(spots[spot]) >= 64
    assert r31 in spots["block"]
    assert (spots["before"] * C + C <= LIM31).all() and (spots["after"] * C >= LIM31).all()  # live rows on both sides
    assert (spots["past"] > r31 + 2 * 256).all() and (spots["past"] // P == B - 1).all()
    assert (spots["last"] >= R - 300).all() and len(spots["last"]) >= 64
    # a dead row everywhere else: most rows of the blocks around 2^31 included
    assert len(rows) < R // 100


@pytest.mark.parametrize("ic", T.IN_CASES, ids=[c.name for c in T.IN_CASES])
def test_conv_input_case_sits_where_its_name_says(ic):
    elems = ic.B * ic.H * ic.W * 64
    x_bytes = elems * 2
    Ho, Wo = T.L.out_hw(ic.H, ic.W, ic.stride)
    assert elems < LIM31 and ic.B * Ho * Wo * ic.Cout < LIM31, "conv_describe must admit the case"
    if ic.name.startswith("below-gate"):
        assert T.GATE - ic.W * 128 <= x_bytes < T.GATE and ic.kernel == "od_conv_8ph<" and ic.Cout > 64
    elif ic.name.startswith("at-gate"):
        assert x_bytes == T.GATE and ic.kernel == "od_conv_igemm<"
    else:
        assert elems == LIM31 - 64 and x_bytes > LIM31 and ic.kernel == "od_conv_igemm<"
    B, H, W = T.IN_REFUSED
    assert B * H * W * 64 == LIM31
    # the patches: inside the image, their reference windows disjoint, stride-aligned, and where the docstring says
    pts = T.input_patches(ic)
    assert (0, 0, 0) in pts and (ic.B - 1, ic.H - T.PATCH, ic.W - T.PATCH) in pts
    wins = []
    for b, y, x in pts:
        assert 0 <= b < ic.B and 0 <= y <= ic.H - T.PATCH and 0 <= x <= ic.W - T.PATCH
        y0, y1, x0, x1 = T.patch_window(ic, y, x)
        assert y0 % 2 == 0 and x0 % 2 == 0 and y0 <= y and x0 <= x and y1 >= y + T.PATCH and x1 >= x + T.PATCH
        assert (y0 == 0 or y - y0 >= T.MARGIN) and (y1 == ic.H or y1 - y - T.PATCH >= T.MARGIN)
        wins.append((b, y0, y1, x0, x1))
    for i, a in enumerate(wins):
        for c in wins[i + 1:]:
            assert a[0] != c[0] or a[2] + 2 <= c[1] or c[2] + 2 <= a[1] or a[4] + 2 <= c[3] or c[4] + 2 <= a[3], "windows touch"
    if x_bytes > LIM31:
        first = [((b * ic.H + y) * ic.W + x) * 128 for b, y, x in pts]
        last = [((b * ic.H + y + T.PATCH - 1) * ic.W + x + T.PATCH - 1) * 128 + 127 for b, y, x in pts]
        assert any(f < LIM31 < l for f, l in zip(first, last)), "no patch straddles byte 2^31"
        assert any(f > LIM31 + (1 << 28) for f in first) and max(last) == x_bytes - 1
    # the reference of a window (CPU): finite, and a zero input gives act(bias) rounded once on every channel
    g = T.L.gen_conv(("large-input", ic.Cout, ic.k, ic.stride), 1, 8, 8, 64, ic.Cout, ic.k, ic.stride, "none", "leaky")
    alpha = T.E._alpha("leaky")
    zero = T.L.epilogue(np.zeros((1, 1, 1, ic.Cout)), g.scale, g.bias, "leaky", alpha).ref16.reshape(-1)
    r = T.L.ref_forward(np.zeros((1, 6, 6, 64), np.float16), g.w, g.scale, g.bias, ic.stride, "leaky", alpha, rounding=False)
    assert np.isfinite(zero).all() and (r.ref16 == zero).all()


def test_the_batch_sizes_the_shapes_claim():
    from oracle import postprocess as opp
    assert len(opp.make_priors((320, 320))) == T.P320
    NC, B, P = T.DENSE_SHAPES["wide"]
    assert ((B - 1) * P * (NC + 6) <= LIM31 < B * P * (NC + 6)) and B == 125  # the smallest batch, and its LAST image
    NC, B, P = T.DENSE_SHAPES["wide126"]
    assert LIM31 // (NC + 6) // P == B - 2
    NC, B, P = T.DENSE_SHAPES["loss74"]
    assert NC == 74 and LIM31 // (NC + 6) // P < B - 1
    NC, B, P = T.DENSE_SHAPES["narrow"]
    assert LIM31 // (NC + 6) // P == 63 and B == 66
