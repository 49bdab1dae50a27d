"""Thin per-op wrappers over the C ABI (torch tensors in / out as HBM containers).  Used by the parity tests and
by anything that wants a single kernel rather than the whole plan.  No op here has a CPU implementation."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, desc
from .net import Context, _stream_ptr, pack_layer


def _ctx(t: torch.Tensor) -> Context:
    if not t.is_cuda:
        raise _lib.OdError("object_detector_amd ops need device tensors (MI355X); there is no CPU path")
    return Context.get(t.device)


def _upload(w_ohwi, scale, bias, device, first=False):
    """pack_layer's three host arrays as device tensors."""
    return tuple(torch.from_numpy(a).to(device) for a in pack_layer(w_ohwi, scale, bias, first))


def conv2d(x: torch.Tensor, w_ohwi: np.ndarray, scale: np.ndarray, bias: np.ndarray, stride=1, act=None, alpha=0.0,
           res: torch.Tensor | None = None, res_mode="none", out_f32=False, tile_cfg=-1, out=None,
           out_batch_stride=0, out_pix_stride=0, splitk=1, splitk_ws=None, next_pointwise=None):
    """x f16 [B,H,W,Cin] (device) ; w [Cout,k,k,Cin] host array -> out f16/f32 [B,Ho,Wo,Cout].
    next_pointwise = (w2 [Cout2,1,1,Cout], scale2, bias2, act2, alpha2): the 1x1 layer that consumes `out`
    (od_conv_desc.w2) -> returns (out, out2)."""
    ctx = _ctx(x)
    assert x.dtype == torch.float16 and x.is_contiguous()
    B, H, Wd, Cin = x.shape
    Cout, k = w_ohwi.shape[0], w_ohwi.shape[1]
    layer = _upload(w_ohwi, scale, bias, x.device)
    Ho, Wo = (H + stride - 1) // stride, (Wd + stride - 1) // stride
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
    if splitk != 1 and splitk_ws is None:
        splitk_ws = torch.empty(32 * B * Ho * Wo * Cout, dtype=torch.float32, device=x.device)
    out2 = then = None
    if next_pointwise is not None:
        w2, scale2, bias2, act2, alpha2 = next_pointwise
        assert w2.shape[1:] == (1, 1, Cout)
        out2 = torch.empty((B, Ho, Wo, w2.shape[0]), dtype=torch.float16, device=x.device)
        then = _upload(w2, scale2, bias2, x.device) + (out2, w2.shape[0], act2, alpha2)
    d = desc.conv(x, *layer, out, B, H, Wd, Cin, Cout, k, stride, act, alpha, res=res, res_mode=res_mode, out_f32=out_f32,
                  out_batch_stride=out_batch_stride, out_pix_stride=out_pix_stride, tile_cfg=tile_cfg, then=then,
                  splitk=None if splitk == 1 else (splitk, splitk_ws, splitk_ws.numel() * 4))
    _lib.check(ctx.lib.od_conv2d_fwd(ctx.handle, C.byref(d), _stream_ptr()), "od_conv2d_fwd")
    if splitk != 1:
        out._splitk_ws = splitk_ws  # keep the workspace alive / inspectable
    if next_pointwise is not None:
        torch.cuda.current_stream().synchronize()  # the packed second-layer weights above are temporaries
        return out, out2
    return out


def conv2d_grouped(xs, w_ohwi: np.ndarray, scale: np.ndarray, bias: np.ndarray, act=None, alpha=0.0, out_f32=False,
                   tile_cfg=-1):
    """The same 3x3 stride-1 layer over several maps xs = [f16 [B,H_i,W_i,Cin]] in one call (od_conv_desc.nseg: the
    prediction module shared by the pyramid levels, reference docs/MODEL.md:8) -> [out_i [B,H_i,W_i,Cout]]."""
    ctx = _ctx(xs[0])
    B, Cin = xs[0].shape[0], xs[0].shape[3]
    Cout, k = w_ohwi.shape[0], w_ohwi.shape[1]
    layer = _upload(w_ohwi, scale, bias, xs[0].device)
    outs = [torch.empty(tuple(x.shape[:3]) + (Cout,), dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
            for x in xs]
    for x in xs:
        assert x.dtype == torch.float16 and x.is_contiguous() and x.shape[0] == B and x.shape[3] == Cin
    d = desc.conv_grouped(xs, [tuple(x.shape[1:3]) for x in xs], outs, *layer, B, Cin, Cout, act, alpha, out_f32=out_f32,
                          tile_cfg=tile_cfg, ksize=k)
    _lib.check(ctx.lib.od_conv2d_fwd(ctx.handle, C.byref(d), _stream_ptr()), "od_conv2d_fwd(grouped)")
    torch.cuda.current_stream().synchronize()  # the packed weights above are temporaries
    return outs


def bottleneck(x: torch.Tensor, w1_ohwi: np.ndarray, scale1, bias1, w3_ohwi: np.ndarray, scale3, bias3, act="leaky",
               alpha=0.1):
    """Fused residual block x + act(bn3(conv3x3(act(bn1(conv1x1(x)))))): x f16 [B,H,W,C] -> f16 [B,H,W,C]."""
    ctx = _ctx(x)
    assert x.dtype == torch.float16 and x.is_contiguous()
    B, H, Wd, Cc = x.shape
    assert w1_ohwi.shape == (Cc // 2, 1, 1, Cc) and w3_ohwi.shape == (Cc, 3, 3, Cc // 2)
    out = torch.empty_like(x)
    d = desc.bneck(x, *_upload(w1_ohwi, scale1, bias1, x.device), *_upload(w3_ohwi, scale3, bias3, x.device), out,
                   B, H, Wd, Cc, act, alpha)
    _lib.check(ctx.lib.od_bottleneck_fwd(ctx.handle, C.byref(d), _stream_ptr()), "od_bottleneck_fwd")
    torch.cuda.current_stream().synchronize()  # the packed weights above are temporaries
    return out


def stem(x_u8: torch.Tensor, w0_ohwi: np.ndarray, scale0, bias0, w3_ohwi: np.ndarray, scale3, bias3, act="leaky", alpha=0.1):
    """Fused first two layers: u8 [B,H,W,3] -> f16 [B,H/2,W/2,64] (od_stem_fwd)."""
    ctx = _ctx(x_u8)
    assert x_u8.dtype == torch.uint8 and x_u8.is_contiguous()
    B, H, Wd, _ = x_u8.shape
    assert w0_ohwi.shape == (32, 3, 3, 3) and w3_ohwi.shape == (64, 3, 3, 32)
    out = torch.empty((B, H // 2, Wd // 2, 64), dtype=torch.float16, device=x_u8.device)
    d = desc.stem(x_u8, *_upload(w0_ohwi, scale0, bias0, x_u8.device, first=True),
                  *_upload(w3_ohwi, scale3, bias3, x_u8.device), out, B, H, Wd, act, alpha)
    _lib.check(ctx.lib.od_stem_fwd(ctx.handle, C.byref(d), _stream_ptr()), "od_stem_fwd")
    torch.cuda.current_stream().synchronize()
    return out


def conv_first(x_u8: torch.Tensor, w_ohwi: np.ndarray, scale, bias, act="leaky", alpha=0.1):
    ctx = _ctx(x_u8)
    assert x_u8.dtype == torch.uint8 and x_u8.is_contiguous()
    B, H, Wd, _ = x_u8.shape
    Cout = w_ohwi.shape[0]
    wp, sc, bi = _upload(w_ohwi, scale, bias, x_u8.device, first=True)
    out = torch.empty((B, H, Wd, Cout), dtype=torch.float16, device=x_u8.device)
    _lib.check(ctx.lib.od_conv_first_fwd(ctx.handle, x_u8.data_ptr(), wp.data_ptr(), sc.data_ptr(), bi.data_ptr(),
                                         out.data_ptr(), B, H, Wd, Cout, *desc.act_pair(act, alpha),
                                         _stream_ptr()), "od_conv_first_fwd")
    return out


def upsample2x_add(a: torch.Tensor, up: torch.Tensor):
    ctx = _ctx(a)
    B, H, Wd, Cc = a.shape
    assert tuple(up.shape) == (B, H // 2, Wd // 2, Cc)
    out = torch.empty_like(a)
    _lib.check(ctx.lib.od_upsample2x_add(ctx.handle, a.data_ptr(), up.data_ptr(), out.data_ptr(), B, H, Wd, Cc,
                                         _stream_ptr()), "od_upsample2x_add")
    return out


def decode_locs(locs: torch.Tensor, priors: torch.Tensor, loc_scale=0.1, clip=False):
    """locs f32 [N,P,4] or [P,4] -> boxes, device-side od.pb.decode_locs (reference check_assign.py:27)."""
    ctx = _ctx(locs)
    squeeze = locs.dim() == 2
    l3 = locs.unsqueeze(0) if squeeze else locs
    l3 = l3.contiguous().float()
    N, P, _ = l3.shape
    out = torch.empty_like(l3)
    _lib.check(ctx.lib.od_decode_locs(ctx.handle, l3.data_ptr(), priors.data_ptr(), out.data_ptr(), N, P,
                                      float(loc_scale), int(clip), _stream_ptr()), "od_decode_locs")
    return out[0] if squeeze else out


BOX_MODES = {"smooth_l1": 0, "mse": 1, "giou": 2, "diou": 3, "ciou": 4}  # od_loss_fwd_bwd_iou's box_mode
IOU_BOX_MODES = ("giou", "diou", "ciou")


def check_box_mode(box_mode, priors, num_priors):
    """The argument rules of loss_fwd_bwd (no device needed): a known mode, and for an IoU mode a prior table [P,4]."""
    if box_mode not in BOX_MODES:
        raise ValueError(f"box_mode must be one of {sorted(BOX_MODES)}, got {box_mode!r}")
    if box_mode in IOU_BOX_MODES:
        if priors is None:
            raise ValueError(f"box_mode {box_mode!r} is taken on decoded boxes: pass priors=<f32 [P,4] device tensor>")
        if priors.dim() != 2 or priors.shape[1] != 4 or priors.shape[0] != num_priors:
            raise ValueError(f"priors {tuple(priors.shape)} do not match the {num_priors} rows per image of pred")


OBJ_MODES = {"focal": 0, "qfl": 1, "vfl": 2}  # od_loss_fwd_bwd_quality's obj_mode
QUALITY_MODES = ("iou", "tal")


def check_objectness(objectness, quality, gamma, rows_shape):
    """The argument rules of loss_fwd_bwd's objectness term (no device needed): a known name; a soft mode ("qfl" | "vfl")
    needs quality of shape `rows_shape` = pred.shape[:-1]; "qfl" needs gamma >= 1 (below 1 its gradient is unbounded at
    p = q)."""
    if objectness not in OBJ_MODES:
        raise ValueError(f"objectness must be one of {sorted(OBJ_MODES)}, got {objectness!r}")
    if objectness == "focal":
        return
    if quality is None:
        raise ValueError(f"objectness {objectness!r} needs quality=<f32 {list(rows_shape)} device tensor> (ops.quality_targets)")
    if tuple(quality.shape) != tuple(rows_shape):
        raise ValueError(f"quality {tuple(quality.shape)} does not match the rows {tuple(rows_shape)} of pred")
    if objectness == "qfl" and not float(gamma) >= 1.0:
        raise ValueError(f'objectness "qfl" needs gamma >= 1, got {gamma!r}')


def check_quality_mode(mode, assigned=None, metric=None, gt_boxes=None):
    """The argument rules of quality_targets (no device needed): a known mode, and for "tal" the three tensors of the
    task-aligned assignment (assigned [B,P] i32, metric [B,P] f32, gt_boxes [B,Gmax,4] f32)."""
    if mode not in QUALITY_MODES:
        raise ValueError(f"quality mode must be one of {QUALITY_MODES}, got {mode!r}")
    if mode == "tal":
        missing = [n for n, v in (("assigned", assigned), ("metric", metric), ("gt_boxes", gt_boxes)) if v is None]
        if missing:
            raise ValueError(f'quality mode "tal" needs assigned=, metric= and gt_boxes= of the od_assign_tal call '
                             f'(missing: {", ".join(missing)})')


def quality_targets(pred: torch.Tensor, y: torch.Tensor, priors: torch.Tensor, loc_scale=0.1, mode="iou", assigned=None,
                    metric=None, gt_boxes=None, out: torch.Tensor | None = None):
    """pred, y f32 [B,P,2+NC+4], priors f32 [P,4] -> q f32 [B,P] in [0,1] on assigned rows, 0 elsewhere   (K10b)
    mode "iou": IoU of the row's decoded target box and its decoded predicted box (od_quality_iou).
    mode "tal": TOOD's normalised alignment metric from the outputs of the task-aligned assignment of THIS pred: `assigned`
    i32 [B,P], `metric` f32 [B,P] (PriorBoxes.last_metric), `gt_boxes` f32 [B,Gmax,4] (od_quality_tal)."""
    check_quality_mode(mode, assigned, metric, gt_boxes)
    ctx = _ctx(pred)
    assert pred.dtype == torch.float32 and y.dtype == torch.float32 and pred.is_contiguous() and y.is_contiguous()
    assert priors.dtype == torch.float32 and priors.is_contiguous() and priors.device == pred.device
    B, P, Cc = pred.shape
    assert y.shape == pred.shape and tuple(priors.shape) == (P, 4)
    q = torch.empty((B, P), dtype=torch.float32, device=pred.device) if out is None else out
    assert q.dtype == torch.float32 and tuple(q.shape) == (B, P) and q.is_contiguous()
    if mode == "iou":
        _lib.check(ctx.lib.od_quality_iou(ctx.handle, pred.data_ptr(), y.data_ptr(), priors.data_ptr(), float(loc_scale), B, P,
                                          Cc - 6, q.data_ptr(), _stream_ptr()), "od_quality_iou")
        return q
    assert assigned.dtype == torch.int32 and tuple(assigned.shape) == (B, P) and assigned.is_contiguous()
    assert metric.dtype == torch.float32 and tuple(metric.shape) == (B, P) and metric.is_contiguous()
    assert gt_boxes.dtype == torch.float32 and gt_boxes.dim() == 3 and gt_boxes.shape[0] == B and gt_boxes.shape[2] == 4 \
        and gt_boxes.is_contiguous()
    gmax = gt_boxes.shape[1]
    wsb = ctx.lib.od_quality_tal_workspace_bytes(B, gmax)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=pred.device)
    _lib.check(ctx.lib.od_quality_tal(ctx.handle, pred.data_ptr(), y.data_ptr(), priors.data_ptr(), float(loc_scale),
                                      gt_boxes.data_ptr(), assigned.data_ptr(), metric.data_ptr(), B, P, gmax, Cc - 6,
                                      q.data_ptr(), ws.data_ptr(), wsb, _stream_ptr()), "od_quality_tal")
    return q


def loss_fwd_bwd(pred: torch.Tensor, y: torch.Tensor, num_classes=20, alpha=0.25, gamma=2.0, box_mode="smooth_l1",
                 weights=(1.0, 1.0, 1.0), priors: torch.Tensor | None = None, loc_scale=0.1, objectness="focal",
                 quality: torch.Tensor | None = None):
    """pred, y f32 [B,P,2+NC+4] -> (losses f32 [4] = obj, cls, box, total ; grad f32 like pred)   (K10)
    box_mode "giou" | "diou" | "ciou": 1 - IoU metric of the boxes decoded from the loc columns with `priors` (f32 [P,4] on
    pred's device) and `loc_scale`; "smooth_l1" | "mse" read neither.
    objectness "qfl" | "vfl": quality focal / varifocal loss towards `quality` (f32 [B,P], quality_targets) on the assigned
    rows (od_loss_fwd_bwd_quality); "focal" (the default) is od_loss_fwd_bwd_iou and reads no quality."""
    check_box_mode(box_mode, priors, pred.shape[-2])
    check_objectness(objectness, quality, gamma, pred.shape[:-1])
    ctx = _ctx(pred)
    assert pred.dtype == torch.float32 and y.dtype == torch.float32 and pred.is_contiguous() and y.is_contiguous()
    B, P, Cc = pred.shape
    assert Cc == num_classes + 6 and y.shape == pred.shape
    pr_ptr = None
    if box_mode in IOU_BOX_MODES:
        assert priors.dtype == torch.float32 and priors.is_contiguous() and priors.device == pred.device
        pr_ptr = priors.data_ptr()
    grad = torch.empty_like(pred)
    losses = torch.empty((4,), dtype=torch.float32, device=pred.device)
    wsb = ctx.lib.od_loss_workspace_bytes(B, P)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=pred.device)
    if objectness != "focal":
        assert quality.dtype == torch.float32 and quality.is_contiguous() and quality.device == pred.device
        _lib.check(ctx.lib.od_loss_fwd_bwd_quality(ctx.handle, pred.data_ptr(), y.data_ptr(), pr_ptr, grad.data_ptr(),
                                                   losses.data_ptr(), B, P, num_classes, float(alpha), float(gamma),
                                                   BOX_MODES[box_mode], float(loc_scale), float(weights[0]),
                                                   float(weights[1]), float(weights[2]), quality.data_ptr(),
                                                   OBJ_MODES[objectness], ws.data_ptr(), wsb, _stream_ptr()),
                   "od_loss_fwd_bwd_quality")
        return losses, grad
    _lib.check(ctx.lib.od_loss_fwd_bwd_iou(ctx.handle, pred.data_ptr(), y.data_ptr(), pr_ptr, grad.data_ptr(),
                                           losses.data_ptr(), B, P, num_classes, float(alpha), float(gamma),
                                           BOX_MODES[box_mode], float(loc_scale), float(weights[0]), float(weights[1]),
                                           float(weights[2]), ws.data_ptr(), wsb, _stream_ptr()), "od_loss_fwd_bwd_iou")
    return losses, grad
