"""Device route of `ObjectDetector.predict` (image_decode="device"): the host reads files and parses JPEG headers
(jpeg.py), everything else is decoded / normalised exactly as imageio.load_image does it; a batch is packed into one
pinned buffer, uploaded with one host-to-device copy, and csrc/jpeg.hip decodes and resizes it into the pipeline's
`Net.input`.  The network input is byte-identical to the host route's.

Routes (ObjectDetector.decode_stats counts them):
    "jpeg"      a JPEG of the supported subset: entropy decode, IDCT, upsampling, colour and resize on the device
    "fallback"  any other file: PIL decodes it on the host at its native size, the device resizes it
    "array"     an ndarray: imageio's normalisation on the host, the device resizes it (or copies it at the input size)
With slices (slicing.py) every image is packed once at its own size and od_tiles_resize cuts and resizes its tiles
(BatchDecoder.run_tiles); files are decoded by PIL on the host ("fallback"), arrays count as "array".
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


class _Blob:
    """Host-side layout of one batch's blob: the descriptor array first, then 16-byte aligned chunks; a resample table is
    packed once per (source, destination) length."""

    def __init__(self, descs):
        self.descs, self.chunks, self.tables = descs, [], {}
        self.off = _align(C.sizeof(descs))

    def put(self, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        o = self.off
        self.chunks.append((o, a))
        self.off = _align(o + a.nbytes)
        return o

    def table(self, n_in, n_out):
        """-> (offset, taps per row) of resample.table(n_in, n_out)"""
        if (n_in, n_out) not in self.tables:
            t = resample.table(n_in, n_out)
            self.tables[n_in, n_out] = (self.put(t), t.shape[1] - 2)
        return self.tables[n_in, n_out]


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

    def _upload(self, blob, ws_bytes):
        """Write the packed batch into the pinned buffer and queue its copy to the device on the current stream."""
        descs, total = blob.descs, blob.off
        if self.copied is not None:
            self.copied.synchronize()  # the previous upload out of the pinned buffer
        self.pinned = self._grow(self.pinned, total, lambda n: torch.empty(n, dtype=torch.uint8).pin_memory())
        self.blob = self._grow(self.blob, total, lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
        self.ws = self._grow(self.ws, max(ws_bytes, 16), lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
        host = self.pinned.numpy()
        host[:C.sizeof(descs)] = np.frombuffer(descs, np.uint8)
        for o, a in blob.chunks:
            host[o:o + a.nbytes] = a
        self.blob[:total].copy_(self.pinned[:total], non_blocking=True)
        self.copied = torch.cuda.Event()
        self.copied.record()
        self.descs, self.used = descs, (total, ws_bytes)

    def run(self, items, out: torch.Tensor):
        """Queue upload + decode + resize of `items` (prepare() results) on the current stream into out uint8
        [B,H,W,3]; rows past len(items) are left as they are."""
        B, H, Wd = out.shape[0], out.shape[1], out.shape[2]
        descs = (_lib.ImgDesc * B)()
        blob = _Blob(descs)
        put = blob.put
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
            d.hcoef_off, d.hk = blob.table(d.width, nw)
            d.vcoef_off, d.vk = blob.table(d.height, nh)
        wsb = C.c_longlong()
        _lib.check(self.lib.od_img_workspace_plan(descs, B, C.byref(wsb)), "od_img_workspace_plan")
        self._upload(blob, int(wsb.value))
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        args = (self.ctx.handle, descs, C.c_void_p(self.blob.data_ptr()), B, C.c_void_p(self.blob.data_ptr()), blob.off,
                C.c_void_p(self.ws.data_ptr()), self.ws.numel(), C.c_void_p(out.data_ptr()), H, Wd, st)
        _lib.check(self.lib.od_jpeg_decode_resize(*args), "od_jpeg_decode_resize")
        _lib.check(self.lib.od_rgb_resize(*args), "od_rgb_resize")

    # -- sliced inference (slicing.py): every image sits ONCE in the blob at its own size; od_tiles_resize cuts its tiles ----
    def pack_tiles(self, images, grid, size_hw):
        """Pack uint8 [h,w,3] images, one od_tile_desc per tile (row g*T + t = tile t of image g) and the tiles' resample
        tables into the pinned buffer and queue its upload on the current stream.  -> [(w, h)] of the images."""
        H, Wd = size_hw
        T = grid.T
        N = len(images) * T
        descs = (_lib.TileDesc * N)()
        blob = _Blob(descs)
        sizes = []
        for g, img in enumerate(images):
            h, w = img.shape[:2]
            sizes.append((w, h))
            src = blob.put(img)
            for t, (x0, y0, x1, y1) in enumerate(grid.rects(w, h).tolist()):
                d = descs[g * T + t]
                d.src_off, d.pitch, d.src_w, d.src_h = src, 3 * w, w, h
                d.x0, d.y0, d.x1, d.y1 = x0, y0, x1, y1
                d.hcoef_off, d.hk = blob.table(x1 - x0, Wd)
                d.vcoef_off, d.vk = blob.table(y1 - y0, H)
        wsb = C.c_longlong()
        _lib.check(self.lib.od_tiles_workspace_plan(descs, N, H, Wd, C.byref(wsb)), "od_tiles_workspace_plan")
        self._upload(blob, int(wsb.value))
        return sizes

    def cut_tiles(self, out: torch.Tensor):
        """Queue od_tiles_resize of the batch pack_tiles uploaded on the current stream: row n of out uint8 [B,H,W,3] = tile
        n; rows past the packed tiles are left as they are."""
        N, H, Wd = len(self.descs), out.shape[1], out.shape[2]
        assert N <= out.shape[0]
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.od_tiles_resize(self.ctx.handle, self.descs, C.c_void_p(self.blob.data_ptr()), N,
                                            C.c_void_p(self.blob.data_ptr()), self.used[0], C.c_void_p(self.ws.data_ptr()),
                                            self.ws.numel(), C.c_void_p(out.data_ptr()), H, Wd, st), "od_tiles_resize")

    def run_tiles(self, images, grid, out: torch.Tensor):
        sizes = self.pack_tiles(images, grid, (out.shape[1], out.shape[2]))
        self.cut_tiles(out)
        return sizes

    def sync_rounds(self):
        """Synchronisation rounds the entropy decode of each JPEG of the last batch needed (reads the workspace; waits
        for the device)."""
        torch.cuda.synchronize(self.device)
        ws = self.ws.cpu().numpy()
        return [int(ws[d.state_ws:d.state_ws + 4].view(np.int32)[0]) for d in self.descs if d.kind == _lib.OD_IMG_JPEG]
