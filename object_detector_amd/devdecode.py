"""Device route of `ObjectDetector.predict` (image_decode="device"): the host reads files and parses JPEG headers
(jpeg.py), everything else is decoded / normalised exactly as imageio.load_image does it; a batch is packed into one
pinned buffer, uploaded with one host-to-device copy, and csrc/jpeg.hip decodes and resizes it into the pipeline's
`Net.input`.  The network input is byte-identical to the host route's.

Routes (ObjectDetector.decode_stats counts them):
    "jpeg"      a JPEG of the supported subset: entropy decode, IDCT, upsampling, colour and resize on the device
    "fallback"  any other file: PIL decodes it on the host at its native size, the device resizes it
    "array"     an ndarray: imageio's normalisation on the host, the device resizes it (or copies it at the input size)
"""
from __future__ import annotations

import ctypes as C
import io
import os

import numpy as np
import torch

from . import _lib, jpeg, resample

ROUTES = ("jpeg", "fallback", "array")


def prepare(x, size_hw, keep_aspect):
    """Decode-pool entry: -> (route, payload, (out_w, out_h), letterbox scale).  payload: a jpeg.JpegInfo, or a uint8
    [h,w,3] array the device resizes to (out_w, out_h)."""
    H, Wd = size_hw
    if isinstance(x, (str, os.PathLike)):
        with open(x, "rb") as f:
            data = f.read()
        try:
            info = jpeg.parse(data)
            wh, sc = resample.letterbox_size((info.height, info.width), size_hw, keep_aspect)
            return "jpeg", info, wh, sc
        except jpeg.Fallback:
            from PIL import Image
            img = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), np.uint8)
            route = "fallback"
    else:
        a = np.asarray(x)
        if a.dtype != np.uint8:
            a = np.clip(a, 0, 255).astype(np.uint8)
        if a.shape[:2] == (H, Wd):  # imageio copies it as is, whatever keep_aspect says
            return "array", np.ascontiguousarray(a[..., :3]), (Wd, H), (1.0, 1.0)
        img, route = a[..., :3], "array"
        if img.ndim != 3 or img.shape[2] != 3:  # a layout PIL interprets on its own: take imageio's result as is
            from .imageio import load_image
            out, sc = load_image(a, size_hw, keep_aspect, True)
            return "array", np.ascontiguousarray(out), (Wd, H), sc
    wh, sc = resample.letterbox_size(img.shape[:2], size_hw, keep_aspect)
    return route, np.ascontiguousarray(img), wh, sc


def _align(v, a=16):
    return (v + a - 1) // a * a


class BatchDecoder:
    """One pipeline's buffers: a pinned staging buffer, its device copy and the kernels' workspace.  All three grow
    monotonically; when image sizes repeat, the steady state allocates nothing."""

    def __init__(self, device):
        from .net import Context
        self.device = torch.device(device)
        self.lib = _lib.load()
        self.ctx = Context.get(self.device)
        self.pinned = self.blob = self.ws = None
        self.copied = None  # event: the last upload out of `pinned` has completed
        self.descs = None
        self.used = (0, 0)  # bytes of blob / workspace the last batch used

    @staticmethod
    def _grow(buf, n, make):
        if buf is None or buf.numel() < n:
            return make(max(n, int(1.25 * (0 if buf is None else buf.numel()))))
        return buf

    def run(self, items, out: torch.Tensor):
        """Queue upload + decode + resize of `items` (prepare() results) on the current stream into out uint8
        [B,H,W,3]; rows past len(items) are left as they are."""
        B, H, Wd = out.shape[0], out.shape[1], out.shape[2]
        descs = (_lib.ImgDesc * B)()
        chunks = []
        off = _align(C.sizeof(descs))
        tables = {}

        def put(a):
            nonlocal off
            a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            o = off
            chunks.append((o, a))
            off = _align(off + a.nbytes)
            return o

        def table(n_in, n_out):
            if (n_in, n_out) not in tables:
                t = resample.table(n_in, n_out)
                tables[n_in, n_out] = (put(t), t.shape[1] - 2)
            return tables[n_in, n_out]

        for d, (route, p, (nw, nh), _) in zip(descs, items):
            d.out_w, d.out_h = nw, nh
            if route == "jpeg":
                subs = p.subsequences()
                d.kind, d.width, d.height, d.ncomp = _lib.OD_IMG_JPEG, p.width, p.height, p.ncomp
                (d.samp_h, d.samp_v), d.mcux, d.mcuy, d.n_sub = p.samp[0], p.mcux, p.mcuy, len(subs)
                d.stream_off, d.stream_bytes = put(p.stream), len(p.stream)
                d.sub_off, d.huff_off, d.quant_off = put(subs), put(p.huff), put(p.quant)
            else:
                d.kind, d.height, d.width = _lib.OD_IMG_RGB, p.shape[0], p.shape[1]
                d.src_off = put(p)
            d.hcoef_off, d.hk = table(d.width, nw)
            d.vcoef_off, d.vk = table(d.height, nh)
        wsb = C.c_longlong()
        _lib.check(self.lib.od_img_workspace_plan(descs, B, C.byref(wsb)), "od_img_workspace_plan")
        total = off
        if self.copied is not None:
            self.copied.synchronize()  # the previous upload out of the pinned buffer
        self.pinned = self._grow(self.pinned, total, lambda n: torch.empty(n, dtype=torch.uint8).pin_memory())
        self.blob = self._grow(self.blob, total, lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
        self.ws = self._grow(self.ws, max(int(wsb.value), 16),
                             lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
        host = self.pinned.numpy()
        host[:C.sizeof(descs)] = np.frombuffer(descs, np.uint8)
        for o, a in chunks:
            host[o:o + a.nbytes] = a
        self.blob[:total].copy_(self.pinned[:total], non_blocking=True)
        self.copied = torch.cuda.Event()
        self.copied.record()
        self.descs, self.used = descs, (total, int(wsb.value))
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        args = (self.ctx.handle, descs, C.c_void_p(self.blob.data_ptr()), B, C.c_void_p(self.blob.data_ptr()), total,
                C.c_void_p(self.ws.data_ptr()), self.ws.numel(), C.c_void_p(out.data_ptr()), H, Wd, st)
        _lib.check(self.lib.od_jpeg_decode_resize(*args), "od_jpeg_decode_resize")
        _lib.check(self.lib.od_rgb_resize(*args), "od_rgb_resize")

    def sync_rounds(self):
        """Synchronisation rounds the entropy decode of each JPEG of the last batch needed (reads the workspace; waits
        for the device)."""
        torch.cuda.synchronize(self.device)
        ws = self.ws.cpu().numpy()
        return [int(ws[d.state_ws:d.state_ws + 4].view(np.int32)[0]) for d in self.descs if d.kind == _lib.OD_IMG_JPEG]
