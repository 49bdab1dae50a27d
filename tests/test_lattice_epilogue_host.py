"""CPU halves of tests/test_gpu_conv_epilogue_variants.py: building a case's reference asserts the conditions that make
its f32 arithmetic exact (tests/lattice_ref.py), so every case of that file is checked here without a GPU -- and the
kernel names it expects are checked against the form bench.py's roofline parses."""
import pathlib
import re
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import test_gpu_conv_epilogue_variants as V  # noqa: E402

E = V.E


@pytest.mark.parametrize("case", V.E8_F16_CASES + V.IGEMM_CASES, ids=str)
def test_conditions_forward_f16(case):
    g, r = E.build_fwd(case)
    assert r.ref16.dtype == np.float16 and np.isfinite(r.ref16).all()
    if case[8] == "up2":
        assert g.res.shape[1:3] == (5, 5)


@pytest.mark.parametrize("case", V.E8_F32_CASES + V.UNSPECIALISED_CASES, ids=str)
def test_conditions_forward_f32(case):
    g, r = E.build_fwd(case, out_f32=True)
    assert r.ref32.dtype == np.float32 and np.isfinite(r.ref32).all()


@pytest.mark.parametrize("case", V.E8_PW_CASES, ids=str)
def test_conditions_fused_pointwise(case):
    g, r1, r2 = E.build_pw(case)
    assert r1.ref16.shape[-1] == 256 and r2.ref16.shape[-1] == 128


def test_conditions_grouped():
    g, xs, rs = E.build_grouped(V.E8_GROUPED_CASE)
    assert [x.shape[1:3] for x in xs] == [(10, 10), (6, 6), (4, 4)]


def test_expected_names_keep_the_head_the_benchmark_parses():
    names = [V.expected_name(c)[0] for c in V.E8_F16_CASES]
    names += [V.expected_name(c, out_f32=True)[0] for c in V.E8_F32_CASES]
    names += [V.expected_name(c[:9] + (c[10],), act2=c[9])[0] for c in V.E8_PW_CASES]
    for n in names:
        assert re.match(r"od_conv_8ph<\d+, (\d+)", n), n
    # compiled policies where the plans have them, the run-time instantiation elsewhere
    assert V.expected_name(V.E8_F16_CASES[0])[0] == "od_conv_8ph<3, 4, 5, -1, false, true>"
    assert V.expected_name(V.E8_F32_CASES[0], out_f32=True)[0] == "od_conv_8ph<3, 4, 16, -1, false, true>"
    assert V.expected_name(V.E8_F32_CASES[1], out_f32=True)[0] == "od_conv_8ph<1, 4, -1, -1, false, false>"
    assert V.expected_name(V.UNSPECIALISED_CASES[0], out_f32=True)[0] == "od_conv_8ph<3, 4, -1, -1, false, true>"
    assert V.expected_name(V.IGEMM_CASES[0])[0] == r"od_conv_igemm<64, 64, 64, \d, \d, \d, 1, \d, true, \d, false, 1>"
    assert V.expected_name(V.UNSPECIALISED_CASES[2], out_f32=True)[0].endswith("false, -1>")
    assert V.epi("elu", "up2") == 10 and V.epi("leaky", "none", True) == 17
