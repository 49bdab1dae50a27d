"""The reference's acceptance loop, closed on the GPU: train -> export -> voc_validate.py logs an mAP (reference
voc_validate.py:24-31, README.md:17,22), on generated "shapes" images because VOC07+12 is not available offline
(scripts/_common.shapes_dataset: colour-coded rectangles of five VOC classes on a smooth background, VOC-like sizes).

What this pins that the per-kernel parity tests cannot:
  * the whole training path converges (Generator(on_device=True) -> encode_truth -> loss -> backward -> SGD -> re-pack),
  * export_params() (masters + BatchNorm running statistics) drives the INFERENCE plan to a detector that works:
    mAP(VOC2007) on held-out images far above chance, through the reference's own entry point,
  * with a TRAINED model (separated confidences, unlike random-init weights) the device pipeline and the all-oracle
    pipeline (oracle logits -> oracle conf -> oracle NMS) keep the same boxes,
  * the BatchNorm running statistics equal the torch oracle's.
Parity stays "unpinned by the reference" (SURVEY.md §8c): the oracle is this repo's CPU restatement."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

S, B = 320, 32
STEPS = 1200
OUT = ROOT / "gpurun_out" / "r03_functional_loop.json"


def _record(key, rec):
    OUT.parent.mkdir(parents=True, exist_ok=True)
    cur = json.loads(OUT.read_text()) if OUT.exists() else {}
    cur[key] = rec
    OUT.write_text(json.dumps(cur, indent=1))


@pytest.fixture(scope="module")
def trained(cuda):
    """Train from scratch on 512 generated images: 1200 steps of batch 32 at 320x320 (about 15 s on one MI355X)."""
    import _common
    import train as train_script
    from object_detector_amd import od_gen, weights as W
    from object_detector_amd.trainer import Trainer
    X, y = _common.shapes_dataset(512, seed=0)
    params0 = train_script.init_for_training(W.random_init(seed=2))
    # base network at the full rate: there is no pre-trained Darknet53 offline (docs/MODEL.md:84-90 defaults are unit-tested)
    tr = Trainer(params0, B, (S, S), device=cuda, lr=0.02, momentum=0.9, weight_decay=1e-4, lr_multipliers={"h.": 1.0 / 3.0})
    gen = od_gen.create_generator((S, S), preprocess_input=None, encode_truth=tr.pb.encode_truth_device, device=cuda,
                                  on_device=True, device_cache=True)  # the decoded dataset lives in HBM
    batches, _ = gen.flow(X, y, batch_size=B, data_augmentation=True, shuffle=True, seed=0, prefetch=2)
    hist = tr.fit(batches, STEPS, lr_schedule=train_script.cosine_schedule(0.02, STEPS, 50))
    torch.cuda.synchronize()
    params = tr.export_params()
    tr._poll_nonfinite(wait=True)  # the flags of the last steps are still pending when fit() returns
    skipped = tr.skipped_steps
    del tr, gen, batches
    torch.cuda.empty_cache()
    return params, hist, skipped


def test_training_converges_and_voc_validate_logs_a_high_map(cuda, trained, tmp_path):
    import _common
    from object_detector_amd import weights as W
    from object_detector_amd.priors import DEFAULT_PRIOR_WH
    params, hist, skipped = trained
    assert np.isfinite(hist).all() and skipped == 0
    first, last = float(hist[:3, 3].mean()), float(hist[-50:, 3].mean())
    print(f"total loss: first 3 steps {first:.3f} -> last 50 steps {last:.3f} ({first / last:.1f}x)")
    assert last * 10.0 <= first, (first, last)
    for k in params:  # what export_params() ships to inference, running statistics included
        assert np.isfinite(params[k]).all(), k
    wpath = tmp_path / "trained.npz"
    W.save(wpath, params, meta={"prior_wh": np.asarray(DEFAULT_PRIOR_WH)})
    Xv, yv = _common.shapes_dataset(64, seed=1000)  # held out: another seed
    _common.write_voc_layout(tmp_path / "VOCdevkit", Xv, yv)
    res = tmp_path / "results"
    r = subprocess.run([sys.executable, str(ROOT / "scripts" / "voc_validate.py"), "--vocdevkit-dir", str(tmp_path / "VOCdevkit"),
                        "--result-dir", str(res), "--weights", str(wpath)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in (res / "validate.log").read_text().splitlines() if "mAP=" in ln]
    assert len(line) == 1
    m_all, m07 = (float(line[0].split(tag)[1].split()[0]) for tag in ("mAP=", "mAP(VOC2007)="))
    print(line[0])
    # chance: a detector that has learnt nothing scores ~0 (random-init weights: 0.0-0.3 on this set); five classes, boxes
    # must overlap a ground-truth box of the right class by IoU >= 0.5.  A converged run logs 90+.
    assert m07 >= 80.0 and m_all >= 80.0, line[0]
    # the untrained starting point through the same entry, for the record
    _record("voc_validate", {"train_steps": STEPS, "batch": B, "input": S, "loss_first3": first, "loss_last50": last,
                             "mAP": m_all, "mAP_VOC2007": m07, "held_out_images": len(Xv)})


def test_trained_model_device_pipeline_vs_all_oracle_pipeline(cuda, trained):
    """BASELINE configs[1] shape (32 x 320^2) with the TRAINED weights on held-out images: logits vs the oracle at a realistic
    logit scale, and the kept boxes of the device pipeline vs the ALL-ORACLE pipeline (fp32-storage oracle logits -> oracle
    confidence -> oracle NMS) -- the end-to-end comparison that is uninformative with random-init weights (0 / 32 images equal,
    profiles/r02/fullsize_parity.json: near-degenerate confidences)."""
    import _common
    from object_detector_amd.detector import ObjectDetector
    from object_detector_amd.imageio import load_image
    from oracle import network as onet, nms as onms, postprocess as opost
    from oracle.compare import logit_stats
    params, _hist, _ = trained
    Xv, _yv = _common.shapes_dataset(B, seed=2000)
    x = np.stack([load_image(img, (S, S), False) for img in Xv])
    od = ObjectDetector(params, B, (S, S), use_multi_gpu=False, device=cuda)
    keep, cnt = od.predict_batch_device(torch.from_numpy(x).to(cuda), conf_threshold=0.01)
    torch.cuda.synchronize()
    got = od.net.pred.cpu().numpy()
    pq = onet.f16_weights(params)  # the model the device runs: f16 conv weights (trained masters are f32)
    ref16 = onet.Runner(pq, storage="f16").forward(x)
    ref32 = onet.Runner(pq, storage="f32").forward(x)
    rec = logit_stats(got, ref16, ref32)
    ref_master = onet.Runner(params, storage="f32").forward(x)  # fp32 weights too: adds the weight quantisation
    rec["max_dev_vs_fp32_master_weights"] = float(np.abs(got - ref_master).max())
    rec["rms_dev_vs_fp32_master_weights"] = float(np.sqrt(np.mean((got - ref_master).astype(np.float64) ** 2)))
    keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
    conf_d, boxes_d = od.post.conf.cpu().numpy(), od.post.boxes.cpu().numpy()
    conf_o, boxes_o = opost.head_postprocess(ref32, od.pb.pb_locs, 20)
    same_all, same_conf, jac, n_dev, n_ora = 0, 0, [], [], []
    for b in range(B):
        # identical inputs: bit-exact indices (the claim of record)
        r, *_ = onms.detect_image(conf_d[b], boxes_d[b], K=1024, conf_threshold=0.01, iou_threshold=0.45, max_det=200)
        assert cnt[b] == len(r) and (keep[b, :len(r)] == r).all()
        # end to end against the all-oracle pipeline
        ro, *_ = onms.detect_image(conf_o[b], boxes_o[b], K=1024, conf_threshold=0.01, iou_threshold=0.45, max_det=200)
        same_all += int(len(r) == len(ro) and (r == ro).all())
        cd, co = conf_d[b].reshape(-1), conf_o[b].reshape(-1)
        hi_d, hi_o = r[cd[r] >= 0.3], ro[co[ro] >= 0.3]  # the detections a user sees (voc_evaluate.py:27 uses 0.6)
        same_conf += int(len(hi_d) == len(hi_o) and (hi_d == hi_o).all())
        jac.append(len(np.intersect1d(r, ro)) / max(1, len(np.union1d(r, ro))))
        n_dev.append(int(len(hi_d)))
        n_ora.append(int(len(hi_o)))
    rec.update(images=B, kept_sets_equal_images=same_all, kept_sets_equal_images_conf_ge_0p3=same_conf,
               kept_jaccard_mean=float(np.mean(jac)), kept_jaccard_min=float(np.min(jac)),
               detections_conf_ge_0p3_device=int(np.sum(n_dev)), detections_conf_ge_0p3_oracle=int(np.sum(n_ora)))
    print(json.dumps(rec, indent=1))
    _record("trained_fullsize_32x320", rec)
    # the confident detections are the same boxes in the same order for (nearly) every image; the whole kept list (down to
    # conf 0.01, up to 200 per image) may differ in its low-confidence tail where candidates are closer than the f16 noise
    assert same_conf >= B - 2, rec
    assert rec["kept_jaccard_mean"] >= 0.8, rec
    assert rec["rms_rel_scale"] <= 3e-4 and rec["rms_dev_vs_fp32"] <= 1.15 * rec["rms_f16oracle_vs_fp32"], rec
    assert rec["max_dev_vs_fp32"] <= 1e-3 * rec["logit_scale"], rec  # north_star's "within 1e-3 on logits", at a trained scale


def test_batchnorm_running_statistics_match_the_torch_oracle(cuda):
    """The update Trainer.forward applies to run_mean / run_var (od_bn_stats / od_chan_final<0>, train.hip) -- what
    export_params() ships to inference -- against the float64 torch oracle over three different batches with the parameters
    held fixed (lr 0).  Convention [BUILD-DEFINED, Keras' non-fused BatchNorm]: moving = 0.99 * moving + 0.01 * batch, biased
    batch variance; the shared prediction-module layer is updated once per pyramid level."""
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import BN_MOMENTUM, Trainer
    from oracle import network as onet
    from oracle.train_ref import TorchDetector
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, _x, anns = _setup(cuda, Bs, Ss)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.0, momentum=0.0, loss_scale=256.0)
    xs = [onet.synthetic_images(Bs, Ss, seed=40 + i) for i in range(3)]
    for x in xs:
        tr.step(torch.from_numpy(x).to(cuda), anns)
    torch.cuda.synchronize()
    tr._poll_nonfinite(wait=True)
    assert tr.skipped_steps == 0
    ref = TorchDetector(params).running_stats_after(xs, momentum=BN_MOMENTUM)
    out = tr.export_params()
    worst_m, worst_v = 0.0, 0.0
    for name, (m, v) in ref.items():
        # 3 updates moved the statistics by ~3 % of (batch - initial): compare the MOVEMENT, not the (dominant) initial value
        dm_ref, dv_ref = m - params[name + ".mean"], v - params[name + ".var"]
        dm, dv = out[name + ".mean"] - params[name + ".mean"], out[name + ".var"] - params[name + ".var"]
        em = np.abs(dm - dm_ref).max() / max(np.abs(dm_ref).max(), 1e-12)
        ev = np.abs(dv - dv_ref).max() / max(np.abs(dv_ref).max(), 1e-12)
        worst_m, worst_v = max(worst_m, em), max(worst_v, ev)
        assert em < 2e-2 and ev < 2e-2, (name, em, ev)
    print(f"running statistics: worst relative error of the 3-step movement: mean {worst_m:.2e}, var {worst_v:.2e} (58 layers)")
    assert len(ref) == 58


def test_skipped_step_restores_running_statistics(cuda):
    """an f16 overflow in a forward activation makes the batch statistics (and so the running statistics) non-finite
    before the gradient check can veto the step; the step is skipped AND the running statistics are put back."""
    from object_detector_amd.trainer import Trainer
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, x, anns = _setup(cuda, Bs, Ss)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.01, momentum=0.9, loss_scale=256.0)
    xt = torch.from_numpy(x).to(cuda)
    tr.step(xt, anns)
    torch.cuda.synchronize()
    run0, p0 = tr.run_stats.clone(), tr.params.clone()
    big = tr.view(tr.params, "b.down3", "w")
    keep = big.clone()
    big.fill_(3.0e4)  # z of b.down3 overflows f16 -> Inf statistics -> NaN downstream
    tr._repack()
    tr.step(xt, anns)
    torch.cuda.synchronize()
    assert int(tr.nonfinite.item()) == 1
    assert torch.equal(tr.run_stats, run0), "running statistics of a skipped step were not restored"
    big.copy_(keep)
    assert torch.equal(tr.params, p0)
    tr._repack()
    tr.step(xt, anns)
    torch.cuda.synchronize()
    tr._poll_nonfinite(wait=True)
    assert tr.skipped_steps == 1 and int(tr.nonfinite.item()) == 0
    assert bool(torch.isfinite(tr.run_stats).all()) and not torch.equal(tr.run_stats, run0)


def test_fit_reports_divergence_instead_of_skipping_forever(cuda):
    """A forward pass that overflows f16 (weights in a bad place: what a learning rate too high for the batch size does, measured
    at 16 x 640^2 with a 50-step warm-up) can be cured by no loss scale, and a skipped step never changes the weights: fit() used
    to burn the remaining steps on NaN.  Now it raises after `max_consecutive_skips` skipped steps in a row; the weights of the
    last good step are intact."""
    from object_detector_amd.trainer import Trainer
    from test_gpu_trainer import _setup
    Bs, Ss = 2, 96
    params, x, anns = _setup(cuda, Bs, Ss)
    tr = Trainer(params, Bs, (Ss, Ss), device=cuda, lr=0.01, momentum=0.9, loss_scale=256.0)
    tr.max_consecutive_skips = 6
    xt = torch.from_numpy(x).to(cuda)
    y, _n, _ = tr.pb.encode_batch(anns, return_device=True)

    def batches():
        while True:
            yield xt, y
    hist = tr.fit(batches(), 3)
    assert np.isfinite(hist).all() and not tr.diverged()
    tr.view(tr.params, "b.down3", "w").fill_(3.0e4)  # every forward pass overflows from here on
    tr._repack()
    p0 = tr.params.clone()
    with pytest.raises(RuntimeError, match="training diverged"):
        tr.fit(batches(), 40)
    assert tr.diverged() and tr.skipped_steps >= 6 and torch.equal(tr.params, p0)
