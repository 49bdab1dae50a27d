"""CPU: the host side of the trainer -> detector weight refresh: the od_refresh_layer table builder (net.refresh_layers)
over a trainer layout with no device behind it, the ValueErrors that must fire before anything touches a GPU, and the host
reference of the GPU tests (tests/refresh_ref.py) against what the loader computes from an export_params-shaped dict."""
import numpy as np
import pytest
import torch

import refresh_ref as R
from object_detector_amd import _lib, desc, net as N, weights as W


def _fake_dev(tr, split=()):
    """A Net._dev for `tr`'s architecture out of host tensors: the shapes Net.__init__ makes, no values."""
    dev = {}
    for name, (_n, cin, cout, k, _s, _bn) in tr.specs.items():
        cp, kp = (cout, 32) if name == "b.conv0" else _lib.conv_weight_dims(cout, cin, k)
        dev[name] = (torch.empty((cp, kp), dtype=torch.float16), torch.empty(cp), torch.empty(cp))
        if name in split:
            cp2, kp2 = _lib.conv_weight_dims(cout, 2 * cin, k)
            dev[name + "#split"] = (torch.empty((cp2, kp2), dtype=torch.float16),) + dev[name][1:]
    return dev


def _as_dict(L):
    return {f: getattr(L, f) for f, _t in _lib.RefreshLayer._fields_}


def test_table_builder_covers_every_layer_once():
    tr = R.FakeTrainer(num_classes=7, neck_ch=64, tower=2)
    dev = _fake_dev(tr, N.MIXED_SPLIT)
    table = N.refresh_layers(tr, dev)
    specs = W.layer_specs(7, 64, 2)
    assert len(table) == len(specs) + len(N.MIXED_SPLIT)
    for L, (name, cin, cout, k, _s, bn) in zip(table, specs):  # the layers, once each, in order
        wp, sc, bi = dev[name]
        first = name == "b.conv0"
        assert (L.Cout, L.Cin, L.ksize, L.cin_repeat, L.first, L.has_bn) == (cout, cin, k, 1, int(first), int(bn)), name
        assert (L.Cout_pad, L.Kpad) == ((32, 32) if first else _lib.conv_weight_dims(cout, cin, k)), name
        assert (L.w_dst, L.scale_dst, L.bias_dst) == (wp.data_ptr(), sc.data_ptr(), bi.data_ptr()), name
        assert L.w_offset == tr.seg[(name, "w")][0]
        if bn:
            assert (L.gamma_offset, L.beta_offset) == (tr.seg[(name, "gamma")][0], tr.seg[(name, "beta")][0])
            assert (L.mean_offset, L.var_offset) == (tr._run_off[name], tr._run_off[name] + desc.pad_to(cout, 4))
        else:
            assert name == "h.out" and L.beta_offset == tr.seg[(name, "bias")][0]
    split_keys = [k for k in dev if k.endswith("#split")]  # then one pack-only entry per split layer, in the dict's order
    assert sorted(split_keys) == sorted(n + "#split" for n in N.MIXED_SPLIT)
    for L, name in zip(table[len(specs):], (k[:-len("#split")] for k in split_keys)):
        _n, cin, cout, k, _s, bn = tr.specs[name]
        assert (L.Cout, L.Cin, L.ksize, L.cin_repeat, L.first) == (cout, cin, k, 2, 0), name
        assert (L.Cout_pad, L.Kpad) == _lib.conv_weight_dims(cout, 2 * cin, k)
        assert L.w_dst == dev[name + "#split"][0].data_ptr() and L.scale_dst is None and L.bias_dst is None
        assert L.w_offset == tr.seg[(name, "w")][0]
    # the sources of every entry lie inside the flat buffers
    for L in table:
        assert 0 <= L.w_offset and L.w_offset + L.Cout * L.ksize ** 2 * L.Cin <= tr.n_flat
        assert L.beta_offset + L.Cout <= tr.n_flat and (not L.has_bn or L.var_offset + L.Cout <= tr.n_stats)


def test_table_builder_rejects_another_architecture():
    tr = R.FakeTrainer(num_classes=7, neck_ch=64)
    with pytest.raises(ValueError, match="architecture"):
        N.refresh_layers(tr, _fake_dev(R.FakeTrainer(num_classes=7, neck_ch=64, tower=2)))
    with pytest.raises(ValueError, match="cannot hold"):
        N.refresh_layers(tr, _fake_dev(R.FakeTrainer(num_classes=300, neck_ch=64)))  # h.out: another Cout_pad
    dev = _fake_dev(tr)
    dev.pop("n.lat3")
    with pytest.raises(ValueError, match="architecture"):
        N.refresh_layers(tr, dev)


def test_refresh_from_errors_fire_before_the_gpu():
    """No GPU is needed (and none is touched): the checks run first."""
    from object_detector_amd.detector import ObjectDetector, check_refresh
    arch = (20, 256, 1)
    check_refresh("cuda:0", arch, R.FakeTrainer(), False)
    check_refresh("cuda:0", arch, R.FakeTrainer(ema_decay=0.9), True)
    with pytest.raises(ValueError, match="device"):
        check_refresh("cuda:0", arch, R.FakeTrainer(device="cuda:1"), False)
    for other in (R.FakeTrainer(num_classes=21), R.FakeTrainer(neck_ch=128), R.FakeTrainer(tower=2)):
        with pytest.raises(ValueError, match="architecture"):
            check_refresh("cuda:0", arch, other, False)
    with pytest.raises(ValueError, match="averaged model"):
        check_refresh("cuda:0", arch, R.FakeTrainer(), True)
    od = ObjectDetector.__new__(ObjectDetector)  # the method itself, on an object that has nothing of the device
    od.device, od.arch = torch.device("cuda:0"), arch
    with pytest.raises(ValueError, match="averaged model"):
        od.refresh_from(R.FakeTrainer(), ema=True)
    with pytest.raises(ValueError, match="architecture"):
        od.refresh_from(R.FakeTrainer(num_classes=3))


def test_fit_and_validator_argument_errors():
    from object_detector_amd.trainer import Trainer
    from object_detector_amd.validate import Validator
    for kw in ({"validate_every": 3}, {"validator": lambda tr, step: None}):
        with pytest.raises(ValueError, match="go together"):
            Trainer.fit(object(), iter(()), 0, **kw)  # fails on its arguments, before it reads the trainer
    with pytest.raises(ValueError, match="positive"):
        Trainer.fit(object(), iter(()), 0, validate_every=0, validator=lambda tr, step: None)
    with pytest.raises(ValueError, match="metric"):
        Validator(None, [], [], metric="accuracy")
    with pytest.raises(ValueError, match="coco=True"):
        Validator(None, [], [], metric="coco_AP")
    with pytest.raises(ValueError, match="annotations"):
        Validator(None, [np.zeros((8, 8, 3), np.uint8)], [])


def test_reference_agrees_with_the_loader():
    """refresh_layers' entries + refresh_ref.layer_ref on flat buffers = the arrays Net.__init__ makes from the dict the
    buffers were filled from (its own statements, repeated here: it needs a device), "#split" packs and image layer included."""
    params = W.random_init(5, num_classes=3, neck_ch=64)
    rng = np.random.default_rng(0)
    for k in params:  # weights off the f16 grid, so that the pack rounds
        if k.endswith(".w"):
            params[k] = (params[k] * rng.uniform(0.9, 1.1, params[k].shape)).astype(np.float32)
    tr = R.FakeTrainer(num_classes=3, neck_ch=64)
    flat, stats = tr.flat_from(params)
    dev = _fake_dev(tr, N.MIXED_SPLIT)
    table = N.refresh_layers(tr, dev)
    names = list(tr.specs) + [k for k in dev if k.endswith("#split")]
    assert len(table) == len(names)
    for L, key in zip(table, names):
        name = key.split("#")[0]
        w = params[name + ".w"]
        scale, bias = W.fold_bn(params, name)
        first = name == "b.conv0"
        if first:
            scale = (scale / np.float32(255.0)).astype(np.float32)
        want = N.pack_layer(w, scale, bias, first)
        if key != name:
            want = (N.pack_conv_weight(np.concatenate([w, w], axis=3)),) + want[1:]
        got = R.layer_ref(flat, stats, _as_dict(L))
        for g, x, what in zip(got, want, ("pack", "scale", "bias")):
            assert g.dtype == x.dtype and g.shape == x.shape, (key, what)
            assert np.array_equal(g.view(np.uint16 if what == "pack" else np.uint32),
                                  x.view(np.uint16 if what == "pack" else np.uint32)), (key, what)


def test_coco_ground_truth_takes_the_detectors_class_count():
    """The categories are the detector's classes, not the classes the annotations happen to contain: a 20-class detector
    validated on data that shows classes up to 14 may predict class 19, and tk.data.coco.evaluate refuses a class that is
    not a category."""
    from object_detector_amd.cocoeval import _dets_from_predictions
    from object_detector_amd.detector import ObjectsPrediction
    from object_detector_amd.pb import ObjectsAnnotation
    from object_detector_amd.validate import coco_ground_truth
    y = [ObjectsAnnotation(None, 200, 100, [1, 14], [[0.1, 0.2, 0.5, 0.6], [0.0, 0.0, 1.0, 1.0]], [False, True]),
         ObjectsAnnotation(None, 50, 80, [], np.zeros((0, 4)))]
    gt = coco_ground_truth(y, 20)
    assert gt.category_ids.tolist() == list(range(20)) and len(gt.category_names) == 20
    assert gt.image_ids.tolist() == [0, 1] and gt.ann_image_ids.tolist() == [0, 0] and gt.ann_classes.tolist() == [1, 14]
    np.testing.assert_allclose(gt.ann_bboxes, [[20, 20, 80, 40], [0, 0, 200, 100]], rtol=1e-6)
    assert gt.ann_crowd.tolist() == [False, True] and gt.ann_areas.tolist() == pytest.approx([3200.0, 20000.0], rel=1e-6)
    pred = [ObjectsPrediction([19], [0.5], [[0.1, 0.1, 0.2, 0.2]]), ObjectsPrediction([], [], np.zeros((0, 4)))]
    assert _dets_from_predictions(gt, pred, None).category_ids.tolist() == [19]
    assert coco_ground_truth(y, 15, [f"c{i}" for i in range(15)]).category_names[14] == "c14"
    with pytest.raises(ValueError, match="class names"):
        coco_ground_truth(y, 20, ["a", "b"])
    with pytest.raises(ValueError, match="annotated classes"):
        coco_ground_truth(y, 14)
