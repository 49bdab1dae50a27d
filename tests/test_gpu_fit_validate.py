"""GPU: Trainer.fit(validate_every=..., validator=Validator(...)) on 32 generated shapes images at 64 x 64: the history it
fills, its metrics against the host route (export_params -> new ObjectDetector -> predict -> evaluate) on the same weights
and images -- exactly equal: the weights on the device have the same bits, so the detections are the same --, the
keep_best file, and a twin run without validation that ends with bit-identical buffers and losses."""
import pathlib
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

S, B, STEPS, EVERY = 64, 8, 6, 3
# conf = objectness x softmax over 20 classes: about 0.5 / 20 for random weights, and the first steps of focal loss push the
# objectness down fast; the threshold is low enough that the six-step model still detects something to compare
CONF = 1e-4


def _trainer_and_batches(cuda, X, y):
    from object_detector_amd import od_gen, weights as W
    from object_detector_amd.trainer import Trainer
    tr = Trainer(W.random_init(2), B, (S, S), device=cuda, lr=0.01, momentum=0.9, weight_decay=1e-4, loss_scale=256.0,
                 lr_multipliers={"h.": 1.0 / 3.0}, ema_decay=0.9)
    gen = od_gen.create_generator((S, S), preprocess_input=None, encode_truth=tr.pb.encode_truth_device, device=cuda,
                                  on_device=True, device_cache=True)
    batches, _ = gen.flow(X, y, batch_size=B, data_augmentation=True, shuffle=True, seed=5, prefetch=0)
    return tr, batches


def _state(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr, k).clone() for k in ("params", "mom", "run_stats", "ema", "ema_run_stats")}


@pytest.fixture(scope="module")
def runs(cuda, tmp_path_factory):
    import _common
    import pytoolkit as tk
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.validate import Validator
    X, y = _common.shapes_dataset(32, seed=0, size_range=(96, 128))
    Xv, yv = _common.shapes_dataset(32, seed=1000, size_range=(96, 128))  # held out: another seed
    best = tmp_path_factory.mktemp("fitval") / "best.npz"
    tr, batches = _trainer_and_batches(cuda, X, y)
    od = ObjectDetector.from_trainer(tr, batch_size=B, n_inflight=2)
    v = Validator(od, Xv, yv, conf_threshold=CONF, keep_best=best)
    snaps, lines = {}, []

    def watched(trainer, step):  # what the weights were when each record was made
        rec = v(trainer, step)
        snaps[step] = trainer.export_params(ema=rec["ema"])
        return rec
    hist = tr.fit(batches, STEPS, validate_every=EVERY, validator=watched, log=lines.append)
    state = _state(tr)
    last_pred = v.last_predictions
    # the host route on the weights fit() ended with
    ref = ObjectDetector(tr.export_params(ema=True), B, (S, S), device=cuda, n_inflight=2)
    ref_pred = ref.predict(Xv, conf_threshold=CONF)
    ref_score = tk.data.voc.evaluate(yv, ref_pred)
    # the twin: same seed, same batches, no validation
    tr2, batches2 = _trainer_and_batches(cuda, X, y)
    hist2 = tr2.fit(batches2, STEPS)
    return dict(v=v, hist=hist, state=state, hist2=hist2, state2=_state(tr2), snaps=snaps, lines=lines, best=best,
                last_pred=last_pred, ref_pred=ref_pred, ref_score=ref_score, tr=tr, od=od, Xv=Xv, yv=yv)


def test_history_and_metrics_equal_the_host_route(runs):
    v = runs["v"]
    assert [r["step"] for r in v.history] == [EVERY, 2 * EVERY]
    for r in v.history:
        assert r["ema"] is True and 0.0 <= r["mAP"] <= 1.0 and 0.0 <= r["mAP_VOC"] <= 1.0
    assert len(runs["lines"]) == 2 and all(l.startswith("validation at step") and "mAP_VOC" in l for l in runs["lines"])
    assert runs["od"].refreshed_from == (id(runs["tr"]), True, STEPS)
    got, want = runs["last_pred"], runs["ref_pred"]
    assert len(got) == len(want) == 32 and sum(len(p) for p in want) > 0
    for a, b in zip(got, want):  # the same detections, bit for bit
        assert np.array_equal(a.classes, b.classes) and np.array_equal(a.confs.view(np.uint32), b.confs.view(np.uint32))
        assert np.array_equal(a.bboxes.view(np.uint32), b.bboxes.view(np.uint32))
    last = v.history[-1]
    print(f"validation mAP {last['mAP']!r} mAP_VOC {last['mAP_VOC']!r}; host route {runs['ref_score']!r}")
    assert last["mAP"] == runs["ref_score"]["mAP"] and last["mAP_VOC"] == runs["ref_score"]["mAP_VOC"]


def test_keep_best_file_holds_the_best_step(runs):
    from object_detector_amd import weights as W
    v = runs["v"]
    scores = [r["mAP_VOC"] for r in v.history]
    best_i = int(np.argmax(scores))  # the first of equal scores: only an improvement rewrites the file
    assert v.best_step == v.history[best_i]["step"] and v.best_value == scores[best_i]
    params, meta = W.load(runs["best"])
    assert int(meta["step"]) == v.best_step and float(meta["mAP_VOC"]) == v.best_value
    want = runs["snaps"][v.best_step]
    assert set(params) == set(want)
    for k in want:
        assert np.array_equal(params[k].view(np.uint32), want[k].view(np.uint32)), k
    assert not list(runs["best"].parent.glob("*.tmp*"))


def test_validation_does_not_perturb_training(runs):
    for k, t in runs["state"].items():
        assert torch.equal(t.view(torch.int32), runs["state2"][k].view(torch.int32)), k
    assert np.array_equal(runs["hist"].view(np.uint32), runs["hist2"].view(np.uint32))
    assert runs["hist"].shape == (STEPS, 4) and np.isfinite(runs["hist"]).all()


def test_coco_validation_scores_classes_the_data_never_shows(runs):
    """coco=True with the 20-class detector on data that shows fewer classes than it can predict: the categories are the
    detector's 20, so a detection of a class above every annotated one is scored, not refused.  The images are the
    validation set with every object relabelled as class 0, which makes that case certain as soon as the model predicts
    any other class.  The twelve numbers equal tk.data.coco.evaluate of the host route's predictions."""
    import pytoolkit as tk
    from object_detector_amd.pb import ObjectsAnnotation
    from object_detector_amd.validate import COCO_STAT_NAMES, Validator, coco_ground_truth
    tr, od = runs["tr"], runs["od"]
    Xs, ref = runs["Xv"], runs["ref_pred"]
    ys = [ObjectsAnnotation(a.path, a.width, a.height, np.zeros_like(a.classes), a.bboxes, a.difficults) for a in runs["yv"]]
    gt_top = 0
    assert max(int(p.classes.max()) for p in ref if len(p)) > gt_top
    v = Validator(od, Xs, ys, conf_threshold=CONF, coco=True, metric="coco_AP50")
    assert v._coco_gt.category_ids.tolist() == list(range(20))
    rec = v(tr, STEPS)
    assert max(int(p.classes.max()) for p in v.last_predictions if len(p)) > gt_top  # refused by a count taken from the data
    keys = ["coco_" + n for n in COCO_STAT_NAMES]
    assert len(keys) == 12 and all(k in rec and np.isfinite(rec[k]) and -1.0 <= rec[k] <= 1.0 for k in keys)
    assert v.best_value == rec["coco_AP50"] and v.best_step == STEPS
    want = tk.data.coco.evaluate(coco_ground_truth(ys, 20), ref, device=od.device).stats
    print("coco stats", [rec[k] for k in keys])
    assert [rec[k] for k in keys] == [float(x) for x in want]


def test_fit_wants_both_arguments_or_neither(runs):
    tr = runs["tr"]
    p0 = tr.params.clone()
    with pytest.raises(ValueError, match="go together"):
        tr.fit(iter(()), 1, validate_every=3)
    with pytest.raises(ValueError, match="go together"):
        tr.fit(iter(()), 1, validator=runs["v"])
    assert torch.equal(tr.params, p0) and len(runs["v"].history) == 2


def test_resume_best_keeps_a_better_file(runs, tmp_path):
    """A validator that takes over an existing keep_best file (a resumed run) leaves it alone until a score is above the
    one it recorded; without resume_best() the first validation starts a new file."""
    from object_detector_amd import weights as W
    from object_detector_amd.validate import Validator, write_params_atomically
    tr, od = runs["tr"], runs["od"]
    path = tmp_path / "best.npz"
    write_params_atomically(path, {"marker.w": np.ones((1, 1, 1, 1), np.float32)}, {"step": np.int64(3), "mAP_VOC": np.float64(2.0)})
    v = Validator(od, runs["Xv"], runs["yv"], conf_threshold=CONF, keep_best=path)
    assert v.resume_best() and (v.best_step, v.best_value) == (3, 2.0)
    v(tr, STEPS)  # no mAP reaches 2.0
    assert set(W.load(path)[0]) == {"marker.w"} and v.best_step == 3
    v2 = Validator(od, runs["Xv"], runs["yv"], conf_threshold=CONF, keep_best=path)
    v2(tr, STEPS)
    assert "h.out.w" in W.load(path)[0] and v2.best_step == STEPS
    assert not Validator(od, [], [], keep_best=tmp_path / "none.npz").resume_best()
