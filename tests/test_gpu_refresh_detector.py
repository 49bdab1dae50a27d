"""GPU: ObjectDetector.refresh_from(trainer) against the host route it replaces -- ObjectDetector(trainer.export_params())
-- at 2 x 64^2: every tensor of net._dev bit for bit, identical logits and kept detections; raw and averaged weights, the
f16 and the mixed plan (split packs); ordering against a batch in flight with no host synchronisation; a plan captured
before the refresh; the argument errors."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 2, 64
CONF = 0.01


def _images(seed):
    return np.random.default_rng(seed).integers(0, 256, (B, S, S, 3), dtype=np.uint8)


def _annotations(seed, nc=20):
    from object_detector_amd.pb import ObjectsAnnotation
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        n = int(rng.integers(1, 4))
        c, wh = rng.uniform(0.25, 0.75, (n, 2)), rng.uniform(0.2, 0.5, (n, 2))
        out.append(ObjectsAnnotation(None, S, S, rng.integers(0, nc, n),
                                     np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1).astype(np.float32)))
    return out


def _step(tr, cuda, seed):
    tr.step(torch.from_numpy(_images(seed)).to(cuda), annotations=_annotations(seed, tr.num_classes))


@pytest.fixture(scope="module")
def trained(cuda):
    """A trainer with an averaged model, three steps away from W.random_init(2) (shared, never stepped again here)."""
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import Trainer
    tr = Trainer(W.random_init(2), B, (S, S), device=cuda, lr=0.02, loss_scale=256.0, ema_decay=0.9)
    for i in range(3):
        _step(tr, cuda, 10 + i)
    tr._poll_nonfinite(wait=True)
    torch.cuda.synchronize()
    assert tr.skipped_steps == 0 and tr.steps_issued == 3
    assert not torch.equal(tr.ema, tr.params)
    return tr


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _assert_same_weights(od, ref, what):
    assert list(od.net._dev) == list(ref.net._dev)
    for key, got in od.net._dev.items():
        for g, w, part in zip(got, ref.net._dev[key], ("pack", "scale", "bias")):
            assert g.shape == w.shape and g.dtype == w.dtype, (what, key, part)
            assert torch.equal(_bits(g), _bits(w)), f"{what}: {key} {part} differs from the host route"


def _run(od, x):
    keep, cnt = od.predict_batch_device(x, conf_threshold=CONF)
    torch.cuda.synchronize()
    return od.net.pred.clone(), keep.clone(), cnt.clone()


def _assert_same_result(a, b, what):
    assert torch.equal(_bits(a[0]), _bits(b[0])), f"{what}: logits differ"
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]), f"{what}: kept detections differ"


@pytest.mark.parametrize("precision", ["f16", "mixed"])
def test_refresh_equals_host_route(cuda, trained, precision):
    from object_detector_amd import weights as W
    from object_detector_amd.detector import ObjectDetector
    tr = trained
    x = torch.from_numpy(_images(1)).to(cuda)
    od = ObjectDetector(W.random_init(9), B, (S, S), device=cuda, n_inflight=2, precision=precision)
    assert od.refreshed_from is None
    if precision == "mixed":
        assert sum(k.endswith("#split") for k in od.net._dev) == len(od.net.split) > 0
    stale = od.params
    for ema in (False, True):
        ref = ObjectDetector(tr.export_params(ema=ema), B, (S, S), device=cuda, n_inflight=1, precision=precision)
        od.refresh_from(tr, ema=ema)
        assert od.refreshed_from == (id(tr), ema, 3) and od.params is stale
        _assert_same_weights(od, ref, f"{precision} ema={ema}")
        _assert_same_result(_run(od, x), _run(ref, x), f"{precision} ema={ema}")
        t = od.submit(x, conf_threshold=CONF)  # the second pipeline shares the refreshed tensors
        t = od.submit(x, conf_threshold=CONF)
        keep, cnt = od.collect(t)
        r = _run(ref, x)
        assert t == 1 and torch.equal(cnt, r[2]) and torch.equal(keep, r[1])
    # the two refreshes wrote different weights (the test would pass trivially otherwise)
    raw = ObjectDetector(tr.export_params(), B, (S, S), device=cuda, n_inflight=1, precision=precision)
    assert any(not torch.equal(_bits(a), _bits(b)) for k in raw.net._dev for a, b in zip(raw.net._dev[k], od.net._dev[k]))


def test_refresh_is_ordered_against_batches_in_flight(cuda):
    """submit -> step -> refresh -> submit with no host synchronisation in between: the earlier ticket holds the old
    weights' result, the later one the result of the synchronised sequence (host route after the step).
    A race test, not a proof: the later ticket is ordered behind the refresh by submit()'s own wait on the caller's stream
    whatever refresh_from does with events, so only the earlier ticket exercises the new waits, and a missing wait on a
    pipeline's `done` event would show only when the timing allows it.  The waits themselves are read in refresh_from."""
    from object_detector_amd import weights as W
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.trainer import Trainer
    tr = Trainer(W.random_init(4), B, (S, S), device=cuda, lr=0.02, loss_scale=256.0)
    _step(tr, cuda, 20)
    x = torch.from_numpy(_images(2)).to(cuda)
    od = ObjectDetector(W.random_init(9), B, (S, S), device=cuda, n_inflight=2)
    for _ in range(2):  # stream calibration and first launches happen here, outside the sequence under test
        od.collect(od.submit(x, conf_threshold=CONF))
    old = _run(od, x)
    t0 = od.submit(x, conf_threshold=CONF)
    _step(tr, cuda, 21)
    od.refresh_from(tr)
    t1 = od.submit(x, conf_threshold=CONF)
    k0, c0 = (v.clone() for v in od.collect(t0))
    k1, c1 = (v.clone() for v in od.collect(t1))
    assert t0 != t1
    torch.cuda.synchronize()
    ref = ObjectDetector(tr.export_params(), B, (S, S), device=cuda, n_inflight=1)
    new = _run(ref, x)
    assert torch.equal(c0, old[2]) and torch.equal(k0, old[1]), "the batch in flight saw refreshed weights"
    assert torch.equal(c1, new[2]) and torch.equal(k1, new[1]), "the batch behind the refresh did not see them"
    _assert_same_weights(od, ref, "unsynchronised refresh")
    assert not torch.equal(_bits(old[0]), _bits(new[0]))


def test_captured_graph_runs_the_refreshed_weights(cuda, trained):
    from object_detector_amd import weights as W
    from object_detector_amd.detector import ObjectDetector
    x = torch.from_numpy(_images(3)).to(cuda)
    od = ObjectDetector(W.random_init(9), B, (S, S), device=cuda, n_inflight=1)
    od.predict_batch_device(x, conf_threshold=CONF, graph=True)  # captured on the old weights
    torch.cuda.synchronize()
    old = od.net.pred.clone()
    assert od.net._captured
    od.refresh_from(trained)
    keep, cnt = od.predict_batch_device(x, conf_threshold=CONF, graph=True)
    torch.cuda.synchronize()
    ref = ObjectDetector(trained.export_params(), B, (S, S), device=cuda, n_inflight=1)
    want = _run(ref, x)
    _assert_same_result((od.net.pred, keep, cnt), want, "replayed graph")
    assert not torch.equal(_bits(old), _bits(want[0]))


def test_from_trainer_and_argument_errors(cuda, trained):
    from object_detector_amd import weights as W
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.trainer import Trainer
    tr3 = Trainer(W.random_init(6, num_classes=3), B, (S, S), device=cuda)  # another class count, no averaged model
    od3 = ObjectDetector.from_trainer(tr3, n_inflight=1)
    assert od3.refreshed_from == (id(tr3), False, 0) and od3.batch_size == B and od3.input_size == (S, S)
    before = {k: tuple(t.clone() for t in v) for k, v in od3.net._dev.items()}
    od3.refresh_from(tr3)  # the host route and the refresh agree on untouched weights too
    torch.cuda.synchronize()
    for k, v in od3.net._dev.items():
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(v, before[k])), k
    with pytest.raises(ValueError, match="averaged model"):
        od3.refresh_from(tr3, ema=True)
    with pytest.raises(ValueError, match="architecture"):
        od3.refresh_from(trained)
    with pytest.raises(ValueError, match="averaged model"):
        ObjectDetector.from_trainer(tr3, ema=True)
