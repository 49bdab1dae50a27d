"""image_decode="device" on JPEG streams that Pillow's encoder never writes (tests/jpeg_crafted.py, every file valid and
decoded by PIL; tests/test_jpeg_crafted_host.py asserts from the reference side that each group reaches its regime): the
device-written network input equals imageio.load_image byte for byte, and the entropy decode needs exactly the
synchronisation rounds the plain model of tests/jpeg_ref.py counts."""
import pathlib
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import jpeg_crafted  # noqa: E402

from object_detector_amd import devdecode  # noqa: E402
from object_detector_amd.imageio import load_image  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = [((96, 96), False), ((96, 96), True), ((320, 320), False), ((320, 320), True)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{group: [(case, path)]}: every crafted file on disk, as predict() would meet it."""
    d = tmp_path_factory.mktemp("crafted")
    out = {}
    for name in jpeg_crafted.GROUPS:
        out[name] = []
        for case, data in jpeg_crafted.group(name).items():
            p = d / f"{case}.jpg"
            p.write_bytes(data)
            out[name].append((case, str(p)))
    return out


@pytest.mark.parametrize("size,keep_aspect", CONFIGS)
@pytest.mark.parametrize("name", jpeg_crafted.GROUPS)
def test_crafted_files_equal_host_input(cuda, files, name, size, keep_aspect):
    """One batch per group: long blocks, flat shared-table images, distinct tables per component, extreme magnitudes,
    coefficient-domain files (no EOB, three ZRL in a row), header forms, geometry edges, luma sampling (1,2)."""
    cases = files[name]
    items = [devdecode.prepare(p, size, keep_aspect) for _, p in cases]
    assert [it[0] for it in items] == ["jpeg"] * len(cases)
    dec = devdecode.BatchDecoder(cuda)
    out = torch.zeros((len(items),) + tuple(size) + (3,), dtype=torch.uint8, device=cuda)
    dec.run(items, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    rounds = dec.sync_rounds()
    bad = []
    for i, (case, p) in enumerate(cases):
        ref, sc = load_image(p, size, keep_aspect, True)
        assert items[i][3] == sc, case
        if not np.array_equal(got[i], ref):
            diff = np.argwhere(got[i] != ref)
            bad.append(f"{case}: {len(diff)} bytes differ, first {diff[:3].tolist()}")
        want = jpeg_crafted.model_rounds(name, case)
        if rounds[i] != want:
            bad.append(f"{case}: {rounds[i]} sync rounds, the model needs {want}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("size,keep_aspect", CONFIGS)
def test_tall_narrow_arrays_follow_pillows_pass_order(cuda, size, keep_aspect):
    """Image.resize runs the vertical pass first when height > 100 * width and the height shrinks; arrays on both sides
    of that rule go through the device resize (route "array")."""
    shapes = [(1500, 8), (801, 8), (800, 8), (1001, 10), (101, 1), (100, 1), (400, 3), (2000, 19)]  # (h, w)
    X = [np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    items = [devdecode.prepare(x, size, keep_aspect) for x in X]
    assert [it[0] for it in items] == ["array"] * len(X)
    dec = devdecode.BatchDecoder(cuda)
    out = torch.zeros((len(items),) + tuple(size) + (3,), dtype=torch.uint8, device=cuda)
    dec.run(items, out)
    got = out.cpu().numpy()
    for i, x in enumerate(X):
        ref, sc = load_image(x, size, keep_aspect, True)
        assert items[i][3] == sc
        np.testing.assert_array_equal(got[i], ref, err_msg=str(shapes[i]))


def test_flat_images_walk_the_round_loop_deep(cuda, files):
    """The flat files are only synchronised by propagation from subsequence 0: the device reports one round per
    subsequence (4:2:0 56, 4:2:2 75, grey 38), as the model does."""
    cases = files["flat"]
    items = [devdecode.prepare(p, (96, 96), False) for _, p in cases]
    dec = devdecode.BatchDecoder(cuda)
    dec.run(items, torch.zeros((len(items), 96, 96, 3), dtype=torch.uint8, device=cuda))
    rounds = dict(zip([c for c, _ in cases], dec.sync_rounds()))
    n_sub = {c: len(it[1].subsequences()) for (c, _), it in zip(cases, items)}
    print("sync rounds", rounds, "subsequences", n_sub)
    for case in ("flat_420", "flat_422", "flat_grey"):
        assert n_sub[case] >= 32 and n_sub[case] / 2 <= rounds[case] <= n_sub[case] + 1, case
