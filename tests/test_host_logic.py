"""CPU: host-side logic of the product package (no kernels run here): the C ABI library loads and exports every
symbol include/odhip.h declares, prior table, VOC loader/evaluator, score report, generator, API surface."""
import ctypes
import pathlib
import re
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _header_functions():
    txt = (ROOT / "include" / "odhip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(od_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_header_symbol():
    from object_detector_amd import _lib
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    names = _header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/odhip.h but not exported by libodhip.so"
    assert set(names) == set(_lib.EXPORTED_SYMBOLS), set(names) ^ set(_lib.EXPORTED_SYMBOLS)
    lib2 = _lib.load()
    assert lib2.od_version() >= 100
    a, b = _lib.conv_weight_dims(208, 256, 3)
    assert (a, b) == (256, 2304)
    assert _lib.conv_weight_dims(64, 32, 3) == (256, 320)  # K tail padded to the 64-deep step


# Every environment variable the package reads.  Tuning, A/B and debug switches do not belong here: a plan chosen by a
# variable set in the shell is not the plan the tests checked.
ENV_ALLOW_LIST = {
    "OD_PRECISION", "OD_INFLIGHT", "OD_INFLIGHT_CALIBRATE", "OD_DECODE_PROCS", "OD_DECODE_THREADS", "OD_GEN_WORKERS",
    "OD_VOC_WEIGHTS",                                 # user configuration
    "OD_TRAIN_GRAD_PAYLOAD", "OD_TRAIN_BUCKET_MB", "OD_TRAIN_FUSE_BN_STATS",
    "OD_DIST_BACKEND", "OD_BENCH_BACKEND", "RANK", "LOCAL_RANK", "WORLD_SIZE", "HSA_ENABLE_IPC_MODE_LEGACY",
    "OD_FUSE_BLOCKS",                                 # the layer-by-layer reference plan of the fused-block tests
    "OD_ABLATE_OPS", "OD_ALLOW_ABLATION",             # bench.py's timing ablation
    "OD_CONV_RDIRECT_MIN_PIXELS",                     # test hook of the register-direct kernel
}


def test_environment_variables_are_allow_listed():
    pkg = ROOT / "object_detector_amd"
    files = list(pkg.rglob("*.py")) + list((pkg / "csrc").glob("*.hip")) + list((pkg / "csrc").glob("*.h"))
    found = set()
    for f in files:
        txt = f.read_text()
        reads = list(re.finditer(r"(?:getenv|os\.environ(?:\.get|\.setdefault|\.pop)?)\s*[(\[]\s*(?:f?[\"']([^\"']+)[\"']|(\w+))",
                                 txt))
        # any other access ("X" in os.environ, os.environ.copy(), an alias of os.environ, ...) would hide a name
        spans = [m.span() for m in reads]
        for k in re.finditer(r"\b(?:getenv|environ)\b", txt):
            assert any(lo <= k.start() < hi for lo, hi in spans), \
                f"{f.name}:{txt.count(chr(10), 0, k.start()) + 1}: environment access the allow-list cannot read"
        for m in reads:
            name = m.group(1)
            if name is None:  # a module-level constant holding the name
                c = re.search(r"^%s\s*=\s*[\"']([^\"']+)[\"']" % m.group(2), txt, flags=re.M)
                assert c, f"{f.name}: environment variable name {m.group(2)} is not a string constant of the module"
                name = c.group(1)
            found.add(name)
    assert found == ENV_ALLOW_LIST, f"not allow-listed: {sorted(found - ENV_ALLOW_LIST)}; unused: {sorted(ENV_ALLOW_LIST - found)}"


def test_ctypes_structs_match_library_layout():
    """Every ctypes Structure of _lib.py against the library's own description of the struct it mirrors (od_sizeof /
    od_offsetof / od_struct_fields): same size, same field names in the same order, same byte offsets -- and every struct
    typedef of include/odhip.h is covered."""
    from object_detector_amd import _lib
    lib = _lib.load()
    hdr = (ROOT / "include" / "odhip.h").read_text()
    declared = set(re.findall(r"typedef struct (od_[a-z0-9_]+) \{", hdr))
    assert declared == {st.C_NAME for st in _lib.STRUCTS}, declared ^ {st.C_NAME for st in _lib.STRUCTS}
    for st in _lib.STRUCTS:
        name = st.C_NAME.encode()
        assert ctypes.sizeof(st) == lib.od_sizeof(name), st.C_NAME
        buf = ctypes.create_string_buffer(1024)
        n = lib.od_struct_fields(name, buf, 1024)
        fields = buf.value.decode().split(",")
        assert n == len(fields) == len(st._fields_), st.C_NAME
        assert fields == [f[0] for f in st._fields_], (st.C_NAME, fields)
        for f in fields:
            assert getattr(st, f).offset == lib.od_offsetof(name, f.encode()), (st.C_NAME, f)
        # ... and the field list the library reports is the header's, in order
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (st.C_NAME, st.C_NAME), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        hdr_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            decl = re.sub(r"\[[^\]]*\]", "", decl)  # array extents
            names = decl.split(",")
            hdr_fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", names[0].strip())[0])
            hdr_fields += [nm.strip().lstrip("*") for nm in names[1:]]
        assert hdr_fields == fields, (st.C_NAME, hdr_fields, fields)
    assert lib.od_sizeof(b"no_such_struct") == -1 and lib.od_offsetof(b"od_conv_desc", b"nope") == -1


def test_ctypes_prototypes_match_header():
    """Every prototype of _lib._PROTOS against the declaration in include/odhip.h: same number of parameters, and each
    parameter of the same KIND (pointer / int / long long / float / size_t) -- a binding that drifts from the header would
    otherwise pass garbage without any error (ctypes cannot check it)."""
    import ctypes as C
    from object_detector_amd import _lib
    hdr = (ROOT / "include" / "odhip.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", hdr, flags=re.S)
    decls = re.findall(r"\n\s*([A-Za-z_][\w \*]*?)\b(od_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr)
    assert len(decls) >= 60

    def kind_of_c(tp):
        tp = tp.strip()
        if tp == "void" or tp == "":
            return None
        if "*" in tp:
            return "ptr"
        base = re.sub(r"\b[A-Za-z_]\w*$", "", tp).strip() or tp  # drop the parameter name
        base = base.replace("const", "").strip()
        return {"int": "i32", "int32_t": "i32", "float": "f32", "long long": "i64", "size_t": "i64", "long": "i64"}[base]

    def kind_of_ctypes(ct):
        if ct in (C.c_void_p, C.c_char_p) or hasattr(ct, "contents") or hasattr(ct, "_type_") and isinstance(ct._type_, type):
            return "ptr"
        assert ct in (C.c_int, C.c_int32, C.c_float, C.c_longlong, C.c_size_t, C.c_long), ct
        return "f32" if ct is C.c_float else ("i32" if C.sizeof(ct) == 4 else "i64")  # LP64: long / long long / size_t = 8 B

    seen = set()
    for ret, name, params in decls:
        assert name in _lib._PROTOS, name
        res, args = _lib._PROTOS[name]
        cparams = [k for k in (kind_of_c(q) for q in params.split(",")) if k is not None]
        got = [kind_of_ctypes(a) for a in args]
        assert got == cparams, (name, cparams, got)
        rk = ret.replace("const", "").strip()
        want_res = {"int": 4, "size_t": 8, "long": 8, "char*": 8, "char *": 8}[rk]
        assert C.sizeof(res) == want_res and (res is C.c_char_p) == ("char" in rk), (name, rk, res)
        seen.add(name)
    assert seen == set(_lib._PROTOS), set(_lib._PROTOS) ^ seen


def test_integration_md_declarations_match_library():
    """INTEGRATION.md §2, first code block executed VERBATIM (only the library path is made absolute): the documented
    ConvDesc must be the library's od_conv_desc (round 1 shipped a stub four fields short)."""
    from object_detector_amd import _lib
    md = (ROOT / "INTEGRATION.md").read_text()
    blocks = re.findall(r"```python\n(.*?)```", md, flags=re.S)
    ns = {}
    exec(blocks[0].replace('C.CDLL("libodhip.so")', f'C.CDLL({str(_lib.LIB_PATH)!r})'), ns)  # its own asserts run here
    assert [f[0] for f in ns["ConvDesc"]._fields_] == [f[0] for f in _lib.ConvDesc._fields_]
    assert ctypes.sizeof(ns["ConvDesc"]) == ctypes.sizeof(_lib.ConvDesc) == 288
    lib = _lib.load()
    for sym, proto in (("od_conv2d_fwd", _lib._PROTOS["od_conv2d_fwd"]), ("od_nms", _lib._PROTOS["od_nms"]),
                       ("od_topk_scores", _lib._PROTOS["od_topk_scores"]),
                       ("od_head_postprocess", _lib._PROTOS["od_head_postprocess"])):
        doc = getattr(ns["lib"], sym).argtypes
        assert len(doc) == len(proto[1]), sym
        for a, b in zip(doc, proto[1]):
            assert ctypes.sizeof(a) == ctypes.sizeof(b), (sym, a, b)


def test_missing_library_fails_loudly(tmp_path):
    from object_detector_amd import _lib
    with pytest.raises(_lib.OdError, match="no CPU fallback"):
        _lib.load(tmp_path / "libodhip.so")


def test_no_gpu_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from object_detector_amd import _lib
    from object_detector_amd.detector import ObjectDetector
    with pytest.raises(_lib.OdError):
        ObjectDetector.synthetic(1, (64, 64))


def test_product_never_imports_oracle():
    for f in (ROOT / "object_detector_amd").rglob("*.py"):
        assert not re.search(r"^\s*(from|import)\s+oracle\b", f.read_text(), flags=re.M), f
    assert not re.search(r"^\s*(from|import)\s+oracle\b", (ROOT / "pytoolkit" / "__init__.py").read_text(), flags=re.M)


def test_priors_match_oracle_and_layout():
    from object_detector_amd import priors as PR
    from oracle import postprocess as opp
    for size in [(320, 320), (640, 640), (256, 384)]:
        assert (PR.make_priors(size) == opp.make_priors(size)).all()
    pr = PR.make_priors((320, 320))
    assert pr.shape == (16800, 4)
    # level-major, then y, x, prior: first cell's 8 priors share a centre
    c = (pr[:8, :2] + pr[:8, 2:]) / 2
    assert np.allclose(c, c[0]) and np.allclose(c[0], 0.5 / 40)


def test_prior_fit_kmeans():
    from object_detector_amd import priors as PR
    rng = np.random.default_rng(1)
    c = rng.uniform(0.2, 0.8, (600, 2))
    wh = np.exp(rng.uniform(np.log(0.05), np.log(0.9), (600, 2)))
    b = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, 1)
    t = PR.fit(b, (320, 320))
    assert t.shape == (3, 8, 2) and (t > 0).all()
    assert PR.make_priors((320, 320), t).shape == (16800, 4)


def test_weights_roundtrip_and_specs(tmp_path):
    from object_detector_amd import weights as W
    from oracle import network as onet
    specs = W.layer_specs()
    assert specs == onet.layer_specs()
    assert sum(1 for s in specs if s[0].startswith("b.")) == 52  # Darknet53 conv count
    n_backbone = sum(co * ci * k * k for (nm, ci, co, k, s, bn) in specs if nm.startswith("b."))
    assert abs(n_backbone - 40.55e6) < 0.05e6
    flops320 = 0
    h = 320
    for nm, ci, co, k, s, bn in specs:
        if not nm.startswith("b."):
            continue
        h = h // s
        flops320 += 2 * h * h * co * ci * k * k
    assert abs(flops320 - 29.01e9) < 0.02e9
    p = {"a.w": np.ones((2, 1, 1, 8), np.float32), "a.bias": np.zeros(2, np.float32)}
    W.save(tmp_path / "w.npz", p, {"prior_wh": np.ones((3, 8, 2))})
    q, meta = W.load(tmp_path / "w.npz")
    assert set(q) == set(p) and (q["a.w"] == p["a.w"]).all() and meta["prior_wh"].shape == (3, 8, 2)
    prm = W.random_init(2)
    ref = onet.init_weights(2)
    assert all((prm[k] == ref[k]).all() for k in ref) and W.infer_arch(prm) == (20, 256, 1)


def _write_voc(root, n=3):
    from PIL import Image
    base = root / "VOC2007"
    for d in ("Annotations", "JPEGImages", "ImageSets/Main"):
        (base / d).mkdir(parents=True, exist_ok=True)
    ids = []
    for i in range(n):
        name = f"{i:06d}"
        ids.append(name)
        Image.fromarray(np.full((100, 200, 3), 40 * i, np.uint8)).save(base / "JPEGImages" / f"{name}.jpg")
        (base / "Annotations" / f"{name}.xml").write_text(f"""<annotation><filename>{name}.jpg</filename>
<size><width>200</width><height>100</height><depth>3</depth></size>
<object><name>dog</name><difficult>0</difficult><bndbox><xmin>21</xmin><ymin>11</ymin><xmax>120</xmax><ymax>90</ymax></bndbox></object>
<object><name>person</name><difficult>{i % 2}</difficult><bndbox><xmin>101</xmin><ymin>1</ymin><xmax>200</xmax><ymax>100</ymax></bndbox></object>
</annotation>""")
    (base / "ImageSets" / "Main" / "test.txt").write_text("\n".join(ids))


def test_voc_loader(tmp_path):
    import pytoolkit as tk
    _write_voc(tmp_path)
    X, y = tk.data.voc.load_07_test(tmp_path)
    assert len(X) == len(y) == 3 and X[0].stem == "000000" and isinstance(X[0], pathlib.Path)
    a = y[1]
    assert a.classes.tolist() == [tk.data.voc.CLASS_NAMES.index("dog"), tk.data.voc.CLASS_NAMES.index("person")]
    np.testing.assert_allclose(a.bboxes[0], [0.1, 0.1, 0.6, 0.9])
    assert a.difficults.tolist() == [False, True]
    assert len(tk.data.voc.CLASS_NAMES) == 20


def test_voc_evaluate_hand_cases():
    import pytoolkit as tk
    from object_detector_amd.detector import ObjectsPrediction
    from object_detector_amd.pb import ObjectsAnnotation
    gt = [ObjectsAnnotation(None, 100, 100, [0, 0], [[0.1, 0.1, 0.4, 0.4], [0.5, 0.5, 0.9, 0.9]]),
          ObjectsAnnotation(None, 100, 100, [1], [[0.2, 0.2, 0.8, 0.8]])]
    perfect = [ObjectsPrediction([0, 0], [0.9, 0.8], gt[0].bboxes), ObjectsPrediction([1], [0.7], gt[1].bboxes)]
    s = tk.data.voc.evaluate(gt, perfect)
    assert s["mAP"] == pytest.approx(1.0) and s["mAP_VOC"] == pytest.approx(1.0)
    # class 0: detections ranked TP, FP, TP -> prec at recall .5 = 1, at recall 1 = 2/3
    pred = [ObjectsPrediction([0, 0, 0], [0.9, 0.8, 0.7], [gt[0].bboxes[0], [0.0, 0.6, 0.1, 0.7], gt[0].bboxes[1]]),
            ObjectsPrediction([], [], np.zeros((0, 4)))]
    s = tk.data.voc.evaluate(gt, pred)
    ap0_int = 0.5 * 1.0 + 0.5 * (2 / 3)
    ap0_11 = (6 * 1.0 + 5 * (2 / 3)) / 11
    assert s["mAP"] == pytest.approx((ap0_int + 0.0) / 2)
    assert s["mAP_VOC"] == pytest.approx((ap0_11 + 0.0) / 2)
    p, r, f, sup = tk.ml.compute_scores(gt, pred, iou_threshold=0.5, num_classes=2)
    assert p[0] == pytest.approx(2 / 3) and r[0] == pytest.approx(1.0) and sup.tolist() == [2, 1] and r[1] == 0
    lines = []
    tk.ml.print_scores(p, r, f, sup, ["a", "b"], print_fn=lines.append)
    assert len(lines) == 4


def test_generator_host_path(tmp_path):
    """reference check_generator.py:17-22 call shapes; boxes track the pixels through flip/crop."""
    import pytoolkit as tk
    _write_voc(tmp_path)
    X, y = tk.data.voc.load_07_test(tmp_path)
    gen = tk.dl.od.od_gen.create_generator((64, 96), preprocess_input=lambda x: x, encode_truth=None)
    g, steps = gen.flow(X, y, batch_size=2, data_augmentation=True, seed=3)
    assert steps == 2
    for _i, (xb, yb) in zip(range(4), g):
        assert xb.dtype == np.uint8 and xb.shape[1:] == (64, 96, 3) and len(yb) == len(xb)
        for a in yb:
            assert hasattr(a, "classes") and hasattr(a, "bboxes")
            assert (a.bboxes >= 0).all() and (a.bboxes <= 1).all() and (a.bboxes[:, 2:] >= a.bboxes[:, :2]).all()
    from object_detector_amd import od_gen
    p = od_gen.AugParams()
    p.flip, p.crop = True, (0.1, 0.2, 0.9, 1.0)
    b = od_gen.transform_boxes(np.array([[0.1, 0.2, 0.5, 0.6]], np.float32), p)
    np.testing.assert_allclose(b, [[0.5, 0.0, 1.0, 0.5]], atol=1e-6)
    img = tk.ml.plot_objects(xb[0], yb[0].classes, None, yb[0].bboxes, tk.data.voc.CLASS_NAMES)
    tk.ndimage.save(tmp_path / "o" / "x.jpg", img)
    assert (tmp_path / "o" / "x.jpg").exists()


def test_generator_stream_independent_of_worker_count(tmp_path):
    """Decode / host augmentation run on a thread pool with the next batch prefetched; parameters are drawn in index order
    on the calling thread, so the batches are identical for any worker count."""
    import pytoolkit as tk
    from object_detector_amd import od_gen
    _write_voc(tmp_path)
    X, y = tk.data.voc.load_07_test(tmp_path)
    outs = []
    for workers in (1, 4):
        gen = od_gen.create_generator((64, 96), workers=workers)
        g, _steps = gen.flow(X, y, batch_size=2, data_augmentation=True, shuffle=True, seed=11)
        outs.append([next(g) for _ in range(5)])
    for (xa, ya), (xb, yb) in zip(*outs):
        assert np.array_equal(xa, xb) and len(ya) == len(yb)
        for a, b in zip(ya, yb):
            assert np.array_equal(a.bboxes, b.bboxes) and np.array_equal(a.classes, b.classes)


def test_tk_surface_matches_reference_scripts():
    """every tk.* symbol the four reference scripts touch exists."""
    import pytoolkit as tk
    for path in ["better_exceptions", "dl.session", "log.init", "log.trace", "log.get", "tqdm", "ndimage.save",
                 "data.voc.load_07_test", "data.voc.evaluate", "data.voc.CLASS_NAMES", "ml.compute_scores",
                 "ml.print_scores", "ml.plot_objects", "dl.od.ObjectDetector", "dl.od.od_gen.create_generator"]:
        o = tk
        for part in path.split("."):
            o = getattr(o, part)
    OD = tk.dl.od.ObjectDetector
    import inspect
    sig = inspect.signature(OD.load_voc)
    for kw in ("batch_size", "input_size", "keep_aspect", "strict_nms", "use_multi_gpu"):
        assert kw in sig.parameters
    assert "conf_threshold" in inspect.signature(OD.predict).parameters
    with pytest.raises(FileNotFoundError):
        OD.load_voc(batch_size=1, use_multi_gpu=False, weights="/nonexistent/voc.npz")

    @tk.log.trace()
    def f(v):
        return v + 1
    assert f(1) == 2


def test_darknet_backbone_import_roundtrip(tmp_path):
    """weights.load_darknet_backbone reads the published Darknet layout (header, then beta/gamma/mean/var/w per conv,
    OIHW) -- checked by writing a file in that layout from known parameters and reading it back.  The real
    darknet53.conv.74 is not available offline: the folded scale/bias must survive the BatchNorm-epsilon rewrite."""
    from object_detector_amd import weights as W
    src = W.random_init(seed=7)
    p = tmp_path / "d53.weights"
    W.save_darknet_backbone(p, src)
    n_expected = sum(4 * cout + cout * cin * k * k for _n, cin, cout, k, _s, _b in W.backbone_specs())
    # 40 620 640 floats + 20 header bytes = 162 482 580 bytes, the size of the published darknet53.conv.74
    assert n_expected == 40_620_640 and p.stat().st_size == 162_482_580
    got, n = W.load_darknet_backbone(p, W.random_init(seed=9))
    assert n == n_expected
    for name, *_ in W.backbone_specs():
        np.testing.assert_array_equal(got[name + ".w"], src[name + ".w"])
        s0, b0 = W.fold_bn(src, name)
        s1, b1 = W.fold_bn(got, name)
        np.testing.assert_allclose(s1, s0, rtol=2e-6)
        np.testing.assert_allclose(b1, b0, rtol=2e-5, atol=1e-6)
    assert np.array_equal(got["h.out.w"], W.random_init(seed=9)["h.out.w"])  # head untouched
    with open(p, "r+b") as f:
        f.truncate(10_000)
    with pytest.raises(ValueError):
        W.load_darknet_backbone(p)


def test_gradient_buckets_tile_the_flat_buffer():
    """make_buckets (overlapped all-reduce): buckets are contiguous, cover the buffer exactly, never split a layer, come in
    backward order, and all but the last are at least the requested size."""
    from object_detector_amd.trainer import make_buckets
    rng = np.random.default_rng(0)
    for trial in range(50):
        sizes = [int(rng.integers(1, 5000)) * 4 for _ in range(int(rng.integers(1, 40)))]
        layers, off = [], 0
        for i, n in enumerate(sizes):
            layers.append((off, off + n, f"l{i}"))
            off += n
        min_elems = int(rng.integers(1, 30000))
        b = make_buckets(layers, off, min_elems)
        assert b[0][1] == off and b[-1][0] == 0
        assert all(x[0] == y[1] for x, y in zip(b, b[1:]))                     # descending, contiguous
        assert all(hi - lo >= min_elems for lo, hi, _ in b[:-1])
        seen = [n for _lo, _hi, names in b for n in names]
        assert sorted(seen) == sorted(nm for _, _, nm in layers)               # every layer in exactly one bucket
        for lo, hi, names in b:
            assert all(lo <= l0 and h0 <= hi for l0, h0, nm in layers if nm in names)


def test_decode_chunk_into_shared_memory(tmp_path):
    """The decode-worker entry (numpy + PIL only, what OD_DECODE_PROCS workers run) writes resized images at the given
    offsets of a shared staging block and returns the letterbox scales; it must not import torch."""
    import subprocess
    import sys
    from multiprocessing import shared_memory
    from PIL import Image
    from object_detector_amd import imageio
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (50, 100, 3), dtype=np.uint8)
    pth = tmp_path / "a.png"
    Image.fromarray(a).save(pth)
    H, W = 32, 48
    nbytes = H * W * 3
    shm = shared_memory.SharedMemory(create=True, size=3 * nbytes)
    try:
        scales = imageio.decode_chunk_into_shm(shm.name, [0, 2 * nbytes], [str(pth), a], (H, W), True)
        got0 = np.ndarray((H, W, 3), np.uint8, buffer=shm.buf, offset=0).copy()
        got2 = np.ndarray((H, W, 3), np.uint8, buffer=shm.buf, offset=2 * nbytes).copy()
        ref, sc = imageio.load_image(a, (H, W), keep_aspect=True, return_scale=True)
        assert np.array_equal(got0, ref) and np.array_equal(got2, ref)
        assert scales == [sc, sc] and sc == (1.0, 0.75)
    finally:
        imageio._SHM.pop(shm.name, None)
        shm.close()
        shm.unlink()
    r = subprocess.run([sys.executable, "-c", "import sys; import object_detector_amd.imageio; print('torch' in sys.modules)"],
                       capture_output=True, text=True, cwd=str(pathlib.Path(__file__).resolve().parent.parent))
    assert r.stdout.strip() == "False", r.stdout + r.stderr


def test_shapes_dataset_roundtrips_through_a_voc_layout(tmp_path):
    """The generated 'shapes' task (scripts/_common.py: what closes the train -> voc_validate loop offline) written as a
    VOCdevkit directory and read back by tk.data.voc.load_07_test: same pixels (png), same classes, boxes to the pixel."""
    sys.path.insert(0, str(ROOT / "scripts"))
    import _common
    import pytoolkit as tk
    from PIL import Image
    X, y = _common.shapes_dataset(5, seed=3)
    assert len(X) == 5 and all(a.num_objects >= 1 and set(a.classes) <= set(_common.SHAPE_CLASSES) for a in y)
    X2, y2 = _common.shapes_dataset(5, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(X, X2))  # seeded
    _common.write_voc_layout(tmp_path, X, y)
    Xr, yr = tk.data.voc.load_07_test(tmp_path)
    assert len(Xr) == 5
    for img, a, pth, b in zip(X, y, Xr, yr):
        assert np.array_equal(np.asarray(Image.open(pth)), img)
        assert a.classes.tolist() == b.classes.tolist()
        h, w = img.shape[:2]
        np.testing.assert_allclose(b.bboxes * [w, h, w, h], a.bboxes * [w, h, w, h], atol=1e-3)
    # every rectangle is painted in its class colour: the mean colour inside a box is close to the class colour
    for img, a in zip(X, y):
        h, w = img.shape[:2]
        c, bb = int(a.classes[-1]), a.bboxes[-1]  # the last one painted is never covered
        patch = img[int(bb[1] * h) + 2:int(bb[3] * h) - 2, int(bb[0] * w) + 2:int(bb[2] * w) - 2].reshape(-1, 3).mean(0)
        col = np.asarray(_common.SHAPE_COLOURS[_common.SHAPE_CLASSES.index(c)], np.float64)
        assert np.abs(patch / np.linalg.norm(patch) - col / np.linalg.norm(col)).max() < 0.08


def test_training_script_helpers():
    """scripts/train.py: focal-loss prior initialisation of the objectness bias, the cosine schedule; trainer.lr_multiplier with
    the docs/MODEL.md:84-90 table and with an override."""
    sys.path.insert(0, str(ROOT / "scripts"))
    import train as T
    from object_detector_amd import weights as W
    from object_detector_amd.trainer import LR_MULTIPLIERS, lr_multiplier
    p = T.init_for_training(W.random_init(2), prior=0.01)
    b = p["h.out.bias"].reshape(W.NUM_PRIORS, 26)
    obj = 1.0 / (1.0 + np.exp(b[:, 0] - b[:, 1]))
    np.testing.assert_allclose(obj, 0.01, rtol=1e-5)
    assert (b[:, 2:] == 0).all() and p["h.out.w"] is not None
    f = T.cosine_schedule(0.02, 100, 10)
    assert f(0) == pytest.approx(0.002) and f(9) == pytest.approx(0.02) and f(10) == pytest.approx(0.02)
    assert f(99) < 1e-4 and all(f(i) >= f(i + 1) for i in range(10, 99))
    assert LR_MULTIPLIERS == {"b.": 0.01, "h.": 1.0 / 3.0}
    assert lr_multiplier("b.s3.0.a") == 0.01 and lr_multiplier("n.lat5") == 1.0
    assert lr_multiplier("b.s3.0.a", {"h.": 1.0 / 3.0}) == 1.0 and lr_multiplier("h.t0", {"h.": 0.5}) == 0.5


def test_mixed_plan_oracle_is_closer_to_fp32_than_f16_storage():
    """oracle.network.MixedPlan (the CPU restatement of ObjectDetector(precision='mixed')) on a small input: strictly less
    logit error than the f16-storage plan, every component of the plan contributing (the attribution DESIGN.md §5 quotes)."""
    from oracle import network as onet
    params = onet.init_weights(2)
    x = onet.synthetic_images(1, 128, seed=0)
    ref = onet.Runner(params, storage="f32").forward(x)
    rms = lambda a: float(np.sqrt(np.mean((a - ref).astype(np.float64) ** 2)))  # noqa: E731
    e16 = rms(onet.Runner(params, storage="f16").forward(x))
    e_mixed = rms(onet.MixedPlan().runner(params).forward(x))
    e_stream = rms(onet.MixedPlan((4, 5), (), True).runner(params).forward(x))
    e_nofpn = rms(onet.MixedPlan((4, 5), ("n.lat4", "n.lat5", "n.out3", "n.out4", "h.t0", "h.out"), False).runner(params).forward(x))
    assert e_mixed < 0.7 * e16 and e_mixed < e_stream < e16 and e_mixed < e_nofpn
    mp = onet.MixedPlan()
    assert mp.storage("b.s3.1.b") and not mp.storage("b.s4.1.b") and mp.storage("b.down4") and not mp.storage("n.lat5")
    assert mp.operand_f16("b.s4.2.a") and not mp.operand_f16("h.out") and not mp.res_f16("n.lat3") and mp.res_f16("b.s3.0.b")
