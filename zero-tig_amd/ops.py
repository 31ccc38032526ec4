"""Tensor-level wrappers over the C ABI: allocate outputs with torch (plumbing), launch the HIP kernels on the
current stream.  No compute happens in torch here."""
import os

import torch

from .lib import current_stream


def _f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


# partial rows of a statistics pass over a >= 1 Mpixel map (tuning knob)
_NBLK_BIG = int(os.environ.get("ZT_NBLK_BIG", "1024"))

class CV:
    """Channel view of an NHWC fp32 buffer [N,H,W,ld]: channels [off, off+C)."""

    def __init__(self, t, off=0, C=None):
        assert t.dtype in (torch.float32, torch.bfloat16) and t.is_contiguous() and t.dim() == 4
        self.t, self.off = t, off
        self.es = t.element_size()
        self.N, self.H, self.W, self.ld = t.shape
        self.C = self.ld - off if C is None else C
        assert 0 <= off and off + self.C <= self.ld

    @property
    def ptr(self):
        return self.t.data_ptr() + self.es * self.off


def _cv(x):
    return x if isinstance(x, CV) else CV(x)


def _dt(t):
    """storage-type code of the C ABI: 0 = fp32, 1 = bf16"""
    return 1 if t.dtype == torch.bfloat16 else 0


def _pooled_dims(h, w):
    """sizes of levels 1..3 of the correlation pyramid over an h x w map: avg_pool2d(2, 2) floors (corr.py:25-27)"""
    return [(h >> l, w >> l) for l in (1, 2, 3)]


ACT = {None: 0, "none": 0, "relu": 1, "lrelu": 2, "sigmoid": 3, "tanh": 4, "sigmoid_clamp": 5}


class Ops:
    def __init__(self, lib):
        self.lib = lib
        self._slab = {}
        self._tickets = {}

    def _s(self, t):
        return current_stream(t.device)

    # live roofline measurement (bench.py): `self.profile = {"match": {conv geometry tuple: name}, "events": {name: [(e0, e1)]}}`
    # brackets the matching launches with HIP events on the launch stream (torch's current stream IS the launch stream here)
    profile = None

    def _ev_begin(self, name):
        if self.profile is None or name is None:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return (name, e0)

    def _ev_end(self, tok):
        if tok is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.profile["events"].setdefault(tok[0], []).append((tok[1], e1))

    # ---- utils/utils.py:203-230 warp_tensor (x2 fused) ---------------------------------------------------
    def warp2(self, flow, imgA, imgB=None, want_taps=False):
        """flow [1,2,Hf,Wf], imgA/imgB [1,C,H,W] -> warped A, warped B (and int32 taps [H,W,2])."""
        _f32c(flow), _f32c(imgA)
        _, C, H, W = imgA.shape
        Hf, Wf = flow.shape[-2:]
        outA = torch.empty_like(imgA)
        outB = torch.empty_like(imgB) if imgB is not None else None
        taps = torch.empty((H, W, 2), dtype=torch.int32, device=imgA.device) if want_taps else None
        tok = self._ev_begin("warp2")
        self.lib.call("zt_warp2_f32", flow, Hf, Wf, imgA, imgB, outA, outB, taps, C, H, W, self._s(imgA))
        self._ev_end(tok)
        return (outA, outB, taps) if want_taps else (outA, outB)

    # ---- stencils -------------------------------------------------------------------------------------------
    def pair_down(self, x):
        _f32c(x)
        _, C, H, W = x.shape
        o1 = torch.empty((1, C, H // 2, W // 2), dtype=torch.float32, device=x.device)
        o2 = torch.empty_like(o1)
        self.lib.call("zt_pair_down_f32", x, o1, o2, C, H, W, self._s(x))
        return o1, o2

    def pair_down_adj(self, g1, g2, H, W, out=None):
        C = g1.shape[1]
        acc = out is not None
        if out is None:
            out = torch.empty((1, C, H, W), dtype=torch.float32, device=g1.device)
        self.lib.call("zt_pair_down_adj_f32", g1, g2, out, C, H, W, int(acc), self._s(g1))
        return out

    def gauss_taps(self):
        """1-D factor of the reference's 21x21 kernel (utils.py:26-39): sqrt of CDF differences, normalised (host, fp64)."""
        if not hasattr(self, "_taps"):
            import math
            nsig, n = 1.0, 21
            interval = (2 * nsig + 1.0) / n
            xs = [(-nsig - interval / 2.0) + i * (2 * nsig + interval) / n for i in range(n + 1)]
            cdf = [0.5 * (1 + math.erf(v / math.sqrt(2.0))) for v in xs]
            k = [math.sqrt(cdf[i + 1] - cdf[i]) for i in range(n)]
            tot = sum(k)
            self._taps = torch.tensor([v / tot for v in k], dtype=torch.float32)
        return self._taps

    def blur21(self, x, tmp=None):
        _f32c(x)
        _, C, H, W = x.shape
        tmp = torch.empty_like(x) if tmp is None else tmp
        out = torch.empty_like(x)
        self.lib.call("zt_blur21_f32", x, tmp, out, self.gauss_taps(), C, H, W, self._s(x))
        return out

    def blur21_adj(self, g, out=None, tmp=None):
        _, C, H, W = g.shape
        acc = out is not None
        out = torch.empty_like(g) if out is None else out
        tmp = torch.empty_like(g) if tmp is None else tmp
        self.lib.call("zt_blur21_adj_f32", g, tmp, out, self.gauss_taps(), C, H, W, int(acc), self._s(g))
        return out

    def box5_reflect(self, x):
        _, C, H, W = x.shape
        out = torch.empty_like(x)
        self.lib.call("zt_box5_reflect_f32", x, out, C, H, W, self._s(x))
        return out

    def box5_reflect_adj(self, g, scale=1.0, out=None):
        _, C, H, W = g.shape
        acc = out is not None
        out = torch.empty_like(g) if out is None else out
        self.lib.call("zt_box5_reflect_adj_f32", g, out, C, H, W, float(scale), int(acc), self._s(g))
        return out

    def localvar_fwd(self, a, b=None, want_D=True):
        _, C, H, W = a.shape
        D = torch.empty_like(a) if want_D else None
        V = torch.empty_like(a)
        self.lib.call("zt_localvar_fwd_f32", a, b, D, V, C, H, W, self._s(a))
        return D, V

    def localvar_bwd(self, D, gV, sign=1.0, out=None):
        _, C, H, W = D.shape
        acc = out is not None
        out = torch.empty_like(D) if out is None else out
        self.lib.call("zt_localvar_bwd_f32", D, gV, out, C, H, W, float(sign), int(acc), self._s(D))
        return out

    def localvar_fwd_pair(self, a, b):
        """(D, V) of localvar_fwd(a) and of localvar_fwd(b, a) in one launch -> DA, VA, DX, VX"""
        _, C, H, W = a.shape
        DA, VA, DX, VX = (torch.empty_like(a) for _ in range(4))
        self.lib.call("zt_localvar_fwd_pair_f32", a, b, DA, VA, DX, VX, C, H, W, self._s(a))
        return DA, VA, DX, VX

    def localvar_bwd_pair(self, DN, DH2, gV, dH3):
        """dH3 += localvar_bwd(DN, gV, -1); returns dH2x = localvar_bwd(DH2, gV, +1) + localvar_bwd(DN, gV, +1), in one launch"""
        _, C, H, W = DN.shape
        dH2x = torch.empty_like(DN)
        self.lib.call("zt_localvar_bwd_pair_f32", DN, DH2, gV, dH3, dH2x, C, H, W, self._s(DN))
        return dH2x

    def half_bwd(self, u1, u2, g1, g2, H, W):
        """pair_down_adj(g1 - box5_reflect_adj(u1), g2 - box5_reflect_adj(u2)) -> [1,C,H,W] in one launch; g1 / g2 stay as they are"""
        C = u1.shape[1]
        out = torch.empty((1, C, H, W), dtype=torch.float32, device=u1.device)
        self.lib.call("zt_half_bwd_f32", u1, u2, g1, g2, out, C, H, W, self._s(u1))
        return out

    def texture_mask(self, a, b, want_ratio=False):
        _, C, H, W = a.shape
        assert C == 3
        m = torch.empty((1, 1, H, W), dtype=torch.float32, device=a.device)
        r = torch.empty_like(m) if want_ratio else None
        self.lib.call("zt_texture_mask_f32", a, b, m, r, H, W, self._s(a))
        return (m, r) if want_ratio else m

    def ycc_flat(self, x):
        out = torch.empty_like(x)
        self.lib.call("zt_ycc_flat_f32", x, out, x.numel(), self._s(x))
        return out

    # ---- output side (zt_io.hip) ------------------------------------------------------------------------------
    def quantize_u8(self, x, mode=0):
        """[1,3,H,W] fp32 in [0,1] -> uint8 [H,W,3] on the device (mode 0: predict.py save_images truncation; 1: evals.py round)."""
        _f32c(x)
        _, C, H, W = x.shape
        assert C == 3
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
        self.lib.call("zt_quantize_u8_hwc", x, out, H, W, int(mode), self._s(x))
        return out

    def png_sizes(self, H, W):
        """-> (workspace bytes, worst-case stream bytes) of `png_encode` for an H x W frame (host query, no device work)"""
        import ctypes
        ws, cap = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self.lib.call("zt_png_sizes", int(H), int(W), ctypes.byref(ws), ctypes.byref(cap))
        return int(ws.value), int(cap.value)

    def png_encode(self, u8_hwc, out=None, mode=1):
        """uint8 [H,W,3] on the device -> (stream, nbytes): `stream` is a uint8 buffer of worst-case size whose first `nbytes`
        (int32 device scalar, shape [1]) bytes are the zlib stream of the image's Paeth-filtered scanlines -- the IDAT payload of
        the PNG predict.py:101-104 writes.  Nothing synchronises: read `nbytes` after the stream has run.  `out`: a buffer of at
        least `png_sizes(H, W)[1]` bytes to write into.  mode 1: literal-only blocks; mode 2: a block with runs of equal
        filtered bytes is written with run-length matches where that is shorter (never longer than mode 1; same sizes)."""
        assert mode in (1, 2), mode
        assert u8_hwc.dtype == torch.uint8 and u8_hwc.dim() == 3 and u8_hwc.shape[2] == 3 and u8_hwc.is_contiguous()
        H, W = int(u8_hwc.shape[0]), int(u8_hwc.shape[1])
        ws_bytes, cap = self.png_sizes(H, W)
        dev = u8_hwc.device
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= cap and out.device == dev
        nbytes = torch.empty(1, dtype=torch.int32, device=dev)
        self.lib.call("zt_png_encode_u8_mode", u8_hwc, H, W, int(mode), ws, ws_bytes, out, out.numel(), nbytes, self._s(u8_hwc))
        return out, nbytes

    def png_code_lengths(self, hist):
        """257-bin histogram (256 byte values + end-of-block; any integer tensor) -> uint8 [257] code lengths of the encoder's
        length-limited canonical Huffman code (at most 15 bits, Kraft sum exactly 1, 0 for symbols that do not occur)."""
        assert hist.numel() == 257
        h = hist.to(torch.int32).contiguous()
        out = torch.empty(257, dtype=torch.uint8, device=h.device)
        self.lib.call("zt_png_code_lengths", h, out, self._s(h))
        return out

    def _to_tensor_lut(self, dev):
        """the 256-entry ToTensor table (`ingest.to_tensor_lut`) on `dev`, uploaded once"""
        from . import ingest
        cache = self.__dict__.setdefault("_ingest_tables", {})
        if ("lut", str(dev)) not in cache:
            cache[("lut", str(dev))] = torch.from_numpy(ingest.to_tensor_lut()).to(dev)
        return cache[("lut", str(dev))]

    def ingest_u8(self, u8, out=None, size=(1920, 1080)):
        """Decoded frame, uint8 [H0,W0,3] (or [1,H0,W0,3]) on the device -> fp32 [1,3,H,W] in [0,1]: the reference loader's
        `im.resize(size)` (PIL BICUBIC, 8-bit two-pass; skipped when the frame already has that size, as PIL does) followed by
        `ToTensor()` (multi_read_data.py:127-132), bit-identical to the host libraries.  size = (W, H) like PIL; None = keep."""
        from . import ingest
        if u8.dim() == 4:
            assert u8.shape[0] == 1
            u8 = u8[0]
        assert u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[2] == 3 and u8.is_contiguous()
        dev, s = u8.device, self._s(u8)
        H0, W0 = int(u8.shape[0]), int(u8.shape[1])
        W, H = (W0, H0) if size is None else size
        cache = self.__dict__.setdefault("_ingest_tables", {})

        def tables(n_in, n_out):
            key = (n_in, n_out, str(dev))
            if key not in cache:
                coef, bounds, ks = ingest.pil_bicubic_tables(n_in, n_out)
                cache[key] = (torch.from_numpy(coef).to(dev), torch.from_numpy(bounds).to(dev), ks)
            return cache[key]
        cur = u8
        if W0 != W:                                           # Resample.c: horizontal pass first, into an 8-bit image
            coef, bounds, ks = tables(W0, W)
            nxt = torch.empty((H0, W, 3), dtype=torch.uint8, device=dev)
            self.lib.call("zt_resample_u8_hwc", cur, nxt, H0, W0, H0, W, 1, coef, bounds, ks, s)
            cur = nxt
        if H0 != H:
            coef, bounds, ks = tables(H0, H)
            nxt = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            self.lib.call("zt_resample_u8_hwc", cur, nxt, H0, W, H, W, 0, coef, bounds, ks, s)
            cur = nxt
        if out is None:
            out = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        assert tuple(out.shape) == (1, 3, H, W) and out.dtype == torch.float32 and out.is_contiguous()
        self.lib.call("zt_u8hwc_to_planar_f32", cur, out, H, W, self._to_tensor_lut(dev), s)
        return out

    # ---- raw video frames (zt_yuv.hip, 8-bit and deep) -----------------------------------------------------------
    def _yuv_payload(self, payload, fmt):
        fmt.check()
        assert payload.dtype == torch.uint8 and payload.dim() == 1 and payload.is_contiguous() and payload.numel() == fmt.frame_bytes, \
            (payload.dtype, tuple(payload.shape), fmt.frame_bytes)

    def yuv_to_rgb_u8(self, payload, fmt, out=None):
        """Y4M payload (1-D uint8: planes Y, U, V of `fmt`, a `y4m.YuvFormat`) -> uint8 [H,W,3] RGB on the device: chroma
        upsampled for the format's siting and the integer matrix of DESIGN 8d, bit-exact.  8-bit formats only."""
        self._yuv_payload(payload, fmt)
        if fmt.depth > 8:
            raise ValueError("yuv_to_rgb_u8: a %d-bit format has no 8-bit RGB decode (yuv_to_planar_f32 takes it)" % fmt.depth)
        if out is None:
            out = torch.empty((fmt.H, fmt.W, 3), dtype=torch.uint8, device=payload.device)
        assert tuple(out.shape) == (fmt.H, fmt.W, 3) and out.dtype == torch.uint8 and out.is_contiguous()
        self.lib.call("zt_yuv_to_rgb_u8", payload, out, fmt.H, fmt.W, fmt.ss, fmt.siting, fmt.decode_coef(), self._s(payload))
        return out

    def yuv_to_planar_f32(self, payload, fmt, out=None):
        """Y4M payload -> fp32 [1,3,H,W] in [0,1]: `ingest_u8(yuv_to_rgb_u8(payload), size=None)` bit for bit in one pass (no RGB
        intermediate, any H * W).  A deep format (depth > 8): 16-bit levels / 65535 by the definition of DESIGN 8f."""
        self._yuv_payload(payload, fmt)
        dev = payload.device
        if out is None:
            out = torch.empty((1, 3, fmt.H, fmt.W), dtype=torch.float32, device=dev)
        assert tuple(out.shape) == (1, 3, fmt.H, fmt.W) and out.dtype == torch.float32 and out.is_contiguous()
        if fmt.depth > 8:
            self.lib.call("zt_yuv16_to_planar_f32", payload, out, fmt.H, fmt.W, fmt.ss, fmt.siting, fmt.depth, fmt.decode_coef(),
                          self._s(payload))
            return out
        self.lib.call("zt_yuv_to_planar_f32", payload, out, fmt.H, fmt.W, fmt.ss, fmt.siting, fmt.decode_coef(),
                      self._to_tensor_lut(dev), self._s(payload))
        return out

    # ---- float resize (zt_resample.hip) -----------------------------------------------------------------
    def _f64_tables(self, n_in, n_out, dev):
        """the double-precision tables of `ingest.pil_bicubic_tables_f64` on `dev`, uploaded once per (in, out)"""
        from . import ingest
        cache = self.__dict__.setdefault("_resample_tables", {})
        key = (int(n_in), int(n_out), str(dev))
        if key not in cache:
            coef, bounds, ks = ingest.pil_bicubic_tables_f64(int(n_in), int(n_out))
            cache[key] = (torch.from_numpy(coef).to(dev), torch.from_numpy(bounds).to(dev), ks)
        return cache[key]

    def resize_planar_f32(self, x, size, clamp=True, out=None, tmp=None):
        """fp32 [1,C,H,W] -> fp32 [1,C,H',W'], size = (W', H') like PIL: Pillow's BICUBIC resize of a mode-F image per plane
        (double accumulation in tap order, rounded to float after each pass), horizontal pass first, then vertical; a pass whose
        size is unchanged is skipped, as Pillow does.  clamp: the last pass that runs stores min(max(v, 0), 1).  With both sizes
        unchanged the result is a copy into `out`, or `x` itself when `out` is None.  `tmp`: the [1,C,H,W'] intermediate of a
        two-pass resize (a caller that is captured into a graph keeps it)."""
        _f32c(x)
        assert x.dim() == 4 and x.shape[0] == 1, tuple(x.shape)
        _, C, H0, W0 = (int(v) for v in x.shape)
        W, H = (int(v) for v in size)
        assert W > 0 and H > 0, size
        dev, s = x.device, self._s(x)
        if out is not None:
            assert tuple(out.shape) == (1, C, H, W) and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev, \
                (tuple(out.shape), (1, C, H, W))
        if (W, H) == (W0, H0):
            if out is None:
                return x
            out.copy_(x)
            return out
        if out is None:
            out = torch.empty((1, C, H, W), dtype=torch.float32, device=dev)
        assert out.data_ptr() != x.data_ptr()
        cur = x
        if W0 != W:
            coef, bounds, ks = self._f64_tables(W0, W, dev)
            last = H0 == H
            if last:
                nxt = out
            else:
                nxt = torch.empty((1, C, H0, W), dtype=torch.float32, device=dev) if tmp is None else tmp
                assert tuple(nxt.shape) == (1, C, H0, W) and nxt.dtype == torch.float32 and nxt.is_contiguous() and nxt.device == dev
            self.lib.call("zt_resample_planar_f32", cur, nxt, C, H0, W0, W, 1, coef, bounds, ks, int(bool(clamp) and last), s)
            cur = nxt
        if H0 != H:
            coef, bounds, ks = self._f64_tables(H0, H, dev)
            self.lib.call("zt_resample_planar_f32", cur, out, C, H0, W, H, 0, coef, bounds, ks, int(bool(clamp)), s)
        return out

    def sized_bufs(self, fmt, size, dev):
        """the buffers `yuv_to_planar_f32_sized` works in: {"decode": [1,3,H,W], "tmp": [1,3,H,W'] or None}"""
        W, H = (int(v) for v in size)
        two = W != fmt.W and H != fmt.H
        return {"decode": torch.empty((1, 3, fmt.H, fmt.W), dtype=torch.float32, device=dev),
                "tmp": torch.empty((1, 3, fmt.H, W), dtype=torch.float32, device=dev) if two else None}

    def yuv_to_planar_f32_sized(self, payload, fmt, size, out=None, bufs=None):
        """Y4M payload of `fmt` (8-bit or deep) -> fp32 [1,3,H',W'] in [0,1], size = (W', H'): `yuv_to_planar_f32` at the source
        size followed by `resize_planar_f32` (clamped), bit for bit.  `bufs` (of `sized_bufs`) holds the decode buffer and the
        intermediate, so a caller that is captured into a graph keeps stable addresses.  The result never aliases `bufs`."""
        W, H = (int(v) for v in size)
        if bufs is None:
            bufs = self.sized_bufs(fmt, size, payload.device)
        x = self.yuv_to_planar_f32(payload, fmt, out=bufs["decode"])
        if out is None:
            out = torch.empty((1, 3, H, W), dtype=torch.float32, device=payload.device)
        return self.resize_planar_f32(x, (W, H), clamp=True, out=out, tmp=bufs["tmp"])

    def rgb_f32_to_yuv(self, x, fmt, out=None):
        """[1,3,H,W] fp32 in [0,1] -> Y4M payload (1-D uint8) of `fmt`: the levels `quantize_u8(x, 0)` makes (predict.py's
        truncation), converted and chroma-subsampled in the same pass.  A deep format (depth > 8): from the 16-bit levels
        (int)(x * 65535 + 0.5) of DESIGN 8f; the payload is still 1-D uint8, `fmt.frame_bytes` long."""
        _f32c(x)
        fmt.check()
        assert tuple(x.shape) == (1, 3, fmt.H, fmt.W), (tuple(x.shape), fmt)
        if out is None:
            out = torch.empty(fmt.frame_bytes, dtype=torch.uint8, device=x.device)
        assert out.dtype == torch.uint8 and out.dim() == 1 and out.numel() == fmt.frame_bytes and out.is_contiguous()
        if fmt.depth > 8:
            self.lib.call("zt_rgb_f32_to_yuv16", x, out, fmt.H, fmt.W, fmt.ss, fmt.siting, fmt.depth, fmt.encode_coef(), self._s(x))
            return out
        self.lib.call("zt_rgb_f32_to_yuv", x, out, fmt.H, fmt.W, fmt.ss, fmt.siting, fmt.encode_coef(), self._s(x))
        return out

    # ---- scene cuts (zt_scene.hip) ------------------------------------------------------------------------------
    def luma_grid(self, payload, fmt, out=None):
        """Y4M payload of `fmt` (1-D uint8), or its luma plane alone (H * W bytes, 1-D or [H,W]) -> int32 [ceil(H/16), ceil(W/16)]:
        per 16 x 16 cell the sum of max(Y - yo, 0), yo = `fmt.decode_coef()[0]` (at most 65280, the library's uint32).
        A deep format (the luma plane is then 2 * H * W bytes): the same grid over min(Y, m) >> (depth - 8), yo = 16 or 0."""
        fmt.check()
        n = fmt.H * fmt.W * (2 if fmt.depth > 8 else 1)
        assert payload.dtype == torch.uint8 and payload.is_contiguous() and \
            ((payload.dim() == 1 and payload.numel() in (n, fmt.frame_bytes)) or tuple(payload.shape) == (fmt.H, n // fmt.H)), \
            (payload.dtype, tuple(payload.shape), fmt.frame_bytes)
        gh, gw = (fmt.H + 15) // 16, (fmt.W + 15) // 16
        if out is None:
            out = torch.empty((gh, gw), dtype=torch.int32, device=payload.device)
        assert out.numel() == gh * gw and out.dtype == torch.int32 and out.is_contiguous() and out.device == payload.device
        if fmt.depth > 8:
            self.lib.call("zt_luma_grid_u16", payload, fmt.H, fmt.W, fmt.depth, 0 if fmt.full else 16, out, self._s(payload))
            return out
        self.lib.call("zt_luma_grid_u8", payload, fmt.H, fmt.W, int(fmt.decode_coef()[0]), out, self._s(payload))
        return out

    def grid_sad(self, a, b, out=None):
        """two grids of `luma_grid` (int32, same size) -> int64 [2]: sum |a - b|, sum (a + b); `out` is overwritten"""
        assert a.dtype == torch.int32 and b.dtype == torch.int32 and a.is_contiguous() and b.is_contiguous() and \
            a.numel() == b.numel() and a.device == b.device, (a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        if out is None:
            out = torch.empty(2, dtype=torch.int64, device=a.device)
        assert tuple(out.shape) == (2,) and out.dtype == torch.int64 and out.is_contiguous() and out.device == a.device
        self.lib.call("zt_grid_sad_u32", a, b, a.numel(), out, self._s(a))
        return out

    # ---- plane metrics of two payloads (zt_planes.hip) ---------------------------------------------------
    def _plane_ws(self, fmt, dev):
        """the workspaces of `yuv_sse` / `ssim_plane` for one layout on one device, allocated once: {"sse": int64 [3 * nblk],
        "nblk", "ssim": float64 [npartial] (sized for the luma plane at the smaller tile), "npartial"}"""
        cache = self.__dict__.setdefault("_plane_workspaces", {})
        key = (fmt.W, fmt.H, fmt.ss, fmt.depth, str(dev))
        if key not in cache:
            hc, wc = fmt.chroma_shape
            nblk = max(1, min(1024, (fmt.H * fmt.W + 2 * hc * wc) // 8192))
            npartial = max(1, -(-(fmt.H - 6) // 16)) * max(1, -(-(fmt.W - 6) // 64))
            cache[key] = {"sse": torch.empty(3 * nblk, dtype=torch.int64, device=dev), "nblk": nblk,
                          "ssim": torch.empty(npartial, dtype=torch.float64, device=dev), "npartial": npartial}
        return cache[key]

    def yuv_sse(self, pa, pb, fmt, out=None):
        """two Y4M payloads of `fmt` (1-D uint8, `fmt.frame_bytes` each) -> int64 [3] on the device: per plane (Y, U, V) the sum of
        the squared sample differences at the format's depth, exact (a deep sample above 2^depth - 1 counts as 2^depth - 1).
        Nothing synchronises; `out` (int64 [3], e.g. a row of a table) is overwritten."""
        self._yuv_payload(pa, fmt), self._yuv_payload(pb, fmt)
        assert pa.device == pb.device, (pa.device, pb.device)
        if out is None:
            out = torch.empty(3, dtype=torch.int64, device=pa.device)
        assert tuple(out.shape) == (3,) and out.dtype == torch.int64 and out.is_contiguous() and out.device == pa.device
        ws = self._plane_ws(fmt, pa.device)
        self.lib.call("zt_yuv_sse", pa, pb, fmt.H, fmt.W, fmt.ss, fmt.depth, ws["sse"], ws["nblk"], out, self._s(pa))
        return out

    def ssim_plane(self, pa, pb, fmt, plane, out=None):
        """plane 0 / 1 / 2 (Y, U, V) of two Y4M payloads of `fmt` -> float64 [1] on the device: skimage's
        structural_similarity(a, b, data_range=2^depth - 1) of that plane (7x7 uniform window; the plane must be at least 7 x 7).
        Nothing synchronises; `out` (float64 [1], e.g. a cell of a table) is overwritten."""
        self._yuv_payload(pa, fmt), self._yuv_payload(pb, fmt)
        assert pa.device == pb.device and plane in (0, 1, 2), (pa.device, pb.device, plane)
        hc, wc = fmt.chroma_shape
        es = 2 if fmt.depth > 8 else 1
        H, W = (fmt.H, fmt.W) if plane == 0 else (hc, wc)
        off = es * (0 if plane == 0 else fmt.H * fmt.W + (plane - 1) * hc * wc)
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=pa.device)
        assert out.numel() == 1 and out.dtype == torch.float64 and out.is_contiguous() and out.device == pa.device
        ws = self._plane_ws(fmt, pa.device)
        self.lib.call("zt_ssim_plane", pa.data_ptr() + off, pb.data_ptr() + off, H, W, fmt.depth, ws["ssim"], ws["npartial"], out,
                      self._s(pa))
        return out

    # ---- temporal consistency of a frame pair (zt_temporal.hip) -------------------------------------------
    def warp_error(self, cur, prev, fb, ff, out_n=None, out3=None):
        """cur, prev [1,3,H,W]; fb, ff [1,2,Hf,Wf]: the backward (cur -> prev) and forward (prev -> cur) flow in pixels at RAFT's
        padded size (the frame centred: oy = (Hf - H) // 2, ox = (Wf - W) // 2) -> (int64 [1], float64 [3]) on the device: the
        number of pixels that pass the forward-backward test, the sum over them of the squared error against the warped previous
        frame, and over all pixels the sums of the squared frame difference and of the absolute brightness difference.
        Nothing synchronises; `out_n` / `out3` (e.g. cells of a table row) are overwritten."""
        _f32c(cur), _f32c(prev), _f32c(fb), _f32c(ff)
        assert cur.dim() == 4 and cur.shape[0] == 1 and cur.shape[1] == 3 and cur.shape == prev.shape, (cur.shape, prev.shape)
        assert fb.dim() == 4 and fb.shape[0] == 1 and fb.shape[1] == 2 and fb.shape == ff.shape, (fb.shape, ff.shape)
        H, W = int(cur.shape[2]), int(cur.shape[3])
        Hf, Wf = int(fb.shape[2]), int(fb.shape[3])
        assert Hf >= H and Wf >= W and all(t.device == cur.device for t in (prev, fb, ff)), (H, W, Hf, Wf)
        dev = cur.device
        # one 256 x 4 tile per workgroup up to 4096 tiles (1024 workgroups striding over the tiles measured the same)
        nblk = max(1, min(4096, -(-H // 4) * -(-W // 256)))
        ws = self.__dict__.setdefault("_warp_error_workspaces", {})
        key = (nblk, str(dev))
        if key not in ws:
            ws[key] = torch.empty(4 * nblk, dtype=torch.int64, device=dev)
        if out_n is None:
            out_n = torch.empty(1, dtype=torch.int64, device=dev)
        if out3 is None:
            out3 = torch.empty(3, dtype=torch.float64, device=dev)
        assert out_n.numel() == 1 and out_n.dtype == torch.int64 and out_n.is_contiguous() and out_n.device == dev
        assert tuple(out3.shape) == (3,) and out3.dtype == torch.float64 and out3.is_contiguous() and out3.device == dev
        self.lib.call("zt_warp_error_f32", cur, prev, fb, ff, H, W, Hf, Wf, (Hf - H) // 2, (Wf - W) // 2, ws[key], nblk, out_n, out3,
                      self._s(cur))
        return out_n, out3

    # ---- looking at those flows (zt_flowviz.hip) -----------------------------------------------------------
    @staticmethod
    def _flow_window(flow, h, w):
        """a flow [1,2,Hf,Wf] (or [2,Hf,Wf]) and the frame's size inside it -> (H, W, Hf, Wf, oy, ox), centred as in `warp_error`"""
        _f32c(flow)
        assert flow.dim() in (3, 4) and tuple(flow.shape[:-2]) in ((2,), (1, 2)), tuple(flow.shape)
        Hf, Wf = int(flow.shape[-2]), int(flow.shape[-1])
        H, W = Hf if h is None else int(h), Wf if w is None else int(w)
        assert 1 <= H <= Hf and 1 <= W <= Wf, (H, W, Hf, Wf)
        return H, W, Hf, Wf, (Hf - H) // 2, (Wf - W) // 2

    def _radius(self, radius, dev):
        """a radius given as a number or as a device tensor -> float32 [1] on the device (a number is written by a fill, in
        stream order, into a cell of its own)"""
        if torch.is_tensor(radius):
            assert radius.numel() == 1 and radius.dtype == torch.float32 and radius.is_contiguous() and radius.device == dev, \
                (radius.dtype, tuple(radius.shape), radius.device)
            return radius
        return torch.full((1,), float(radius), dtype=torch.float32, device=dev)

    def flow_wheel(self):
        """-> uint8 [55, 3] on the host: the colour wheel the kernels use"""
        out = torch.empty((55, 3), dtype=torch.uint8)
        self.lib.call("zt_flow_wheel", out)
        return out

    def flow_radmax(self, fa, fb=None, h=None, w=None, out=None):
        """the largest finite radius sqrt(u^2 + v^2) over the frame's window (h x w, centred) of one flow or of two ->
        float32 [1] on the device.  Nothing synchronises; `out` is overwritten."""
        H, W, Hf, Wf, oy, ox = self._flow_window(fa, h, w)
        dev = fa.device
        if fb is not None:
            _f32c(fb)
            assert fb.shape == fa.shape and fb.device == dev, (fa.shape, fb.shape)
        nblk = max(1, min(4096, -(-H // 4) * -(-W // 256)))
        ws = self.__dict__.setdefault("_radmax_workspaces", {})
        key = (nblk, str(dev))
        if key not in ws:
            ws[key] = torch.empty(nblk, dtype=torch.float32, device=dev)
        if out is None:
            out = torch.empty(1, dtype=torch.float32, device=dev)
        assert out.numel() == 1 and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev
        self.lib.call("zt_flow_radmax_f32", fa, fb, H, W, Hf, Wf, oy, ox, ws[key], nblk, out, self._s(fa))
        return out

    def flow_to_rgb(self, flow, h=None, w=None, radius=None, u8=False, bgr=False, out=None):
        """the colour wheel of Baker et al. 2007 over the frame's window of a flow -> uint8 [h, w, 3] (u8=True, the layout of the
        reference's `flow_to_image`) or fp32 [1, 3, h, w] of level / 255.  `radius`: the flow drawn at full saturation, a number
        or a float32 [1] on the device; None: this flow's own largest radius (`flow_radmax`).  Nothing synchronises."""
        H, W, Hf, Wf, oy, ox = self._flow_window(flow, h, w)
        dev = flow.device
        rad = self.flow_radmax(flow, h=H, w=W) if radius is None else self._radius(radius, dev)
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if u8 else torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        assert out.dtype == (torch.uint8 if u8 else torch.float32) and out.numel() == 3 * H * W and out.is_contiguous() and \
            out.device == dev, (out.dtype, tuple(out.shape))
        self.lib.call("zt_flow_to_rgb", flow, H, W, Hf, Wf, oy, ox, rad, out if u8 else None, None if u8 else out, int(bool(bgr)),
                      self._s(flow))
        return out

    def tc_viz(self, cur, prev, fb, ff, radius, gain, out=None):
        """the four-panel picture of a frame pair -> fp32 [1, 3, 2H, 2W]: the wheel colours of the backward and of the forward flow
        (both at `radius`, a number or a float32 [1] on the device), the current frame with the pixels that leave the frame in
        magenta and those that fail the forward-backward test in cyan, and sqrt(e / 3) * gain of the valid pixels in grey
        (arguments as `warp_error`).  prev=None (a frame without a partner; fb, ff, radius are ignored): white, white, cur, black.
        Nothing synchronises."""
        _f32c(cur)
        assert cur.dim() == 4 and cur.shape[0] == 1 and cur.shape[1] == 3, cur.shape
        H, W = int(cur.shape[2]), int(cur.shape[3])
        dev = cur.device
        if out is None:
            out = torch.empty((1, 3, 2 * H, 2 * W), dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.numel() == 12 * H * W and out.is_contiguous() and out.device == dev, \
            (out.dtype, tuple(out.shape))
        if prev is None:
            self.lib.call("zt_tc_viz_f32", cur, None, None, None, H, W, H, W, 0, 0, None, float(gain), out, self._s(cur))
            return out
        _f32c(prev), _f32c(fb), _f32c(ff)
        assert prev.shape == cur.shape, (cur.shape, prev.shape)
        assert fb.dim() == 4 and fb.shape[0] == 1 and fb.shape[1] == 2 and fb.shape == ff.shape, (fb.shape, ff.shape)
        Hf, Wf = int(fb.shape[2]), int(fb.shape[3])
        assert Hf >= H and Wf >= W and all(t.device == dev for t in (prev, fb, ff)), (H, W, Hf, Wf)
        self.lib.call("zt_tc_viz_f32", cur, prev, fb, ff, H, W, Hf, Wf, (Hf - H) // 2, (Wf - W) // 2, self._radius(radius, dev),
                      float(gain), out, self._s(cur))
        return out

    def flow_pack(self, flow, h=None, w=None, out=None):
        """the frame's window of a planar padded flow -> fp32 [h, w, 2], u and v interleaved: the payload of a .flo file"""
        H, W, Hf, Wf, oy, ox = self._flow_window(flow, h, w)
        if out is None:
            out = torch.empty((H, W, 2), dtype=torch.float32, device=flow.device)
        assert out.dtype == torch.float32 and out.numel() == 2 * H * W and out.is_contiguous() and out.device == flow.device, \
            (out.dtype, tuple(out.shape))
        self.lib.call("zt_flow_pack_hwc_f32", flow, H, W, Hf, Wf, oy, ox, out, self._s(flow))
        return out

    # ---- evals.py's frame metrics, results left on the device (the video loop reads a table back every 64 frames) -------
    def sqdiff_u8(self, a, b, out=None):
        """the integer of `psnr_u8`: sum (round(a*255) - round(b*255))^2 -> int64 [1] on the device, no read-back"""
        _f32c(a), _f32c(b)
        n = a.numel()
        assert b.numel() == n
        ws = self.__dict__.setdefault("_sqdiff_workspaces", {})
        nblk = max(1, min(1024, n // 4096))
        key = (nblk, str(a.device))
        if key not in ws:
            ws[key] = torch.empty(nblk, dtype=torch.int64, device=a.device)
        if out is None:
            out = torch.empty(1, dtype=torch.int64, device=a.device)
        assert out.numel() == 1 and out.dtype == torch.int64 and out.is_contiguous() and out.device == a.device
        self.lib.call("zt_sqdiff_u8_f32", a, b, n, ws[key], nblk, out, self._s(a))
        return out

    def ssim_u8_dev(self, a, b, out=None):
        """the number of `ssim_u8` -> float64 [1] on the device, no read-back"""
        _f32c(a), _f32c(b)
        assert a.dim() == 4 and a.shape[0] == 1 and a.shape[1] == 3 and a.shape == b.shape, (a.shape, b.shape)
        H, W = int(a.shape[2]), int(a.shape[3])
        npart = 3 * max(1, -(-(H - 6) // 32)) * max(1, -(-(W - 6) // 64))
        ws = self.__dict__.setdefault("_ssim_workspaces", {})
        key = (npart, str(a.device))
        if key not in ws:
            ws[key] = torch.empty(npart, dtype=torch.float64, device=a.device)
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=a.device)
        assert out.numel() == 1 and out.dtype == torch.float64 and out.is_contiguous() and out.device == a.device
        self.lib.call("zt_ssim_u8_f32", a, b, H, W, ws[key], npart, out, self._s(a))
        return out

    # ---- no-reference grading of a frame against its own input (zt_noref.hip) ----------------------------
    def _noref_args(self, a, b, grid):
        _f32c(a), _f32c(b)
        assert a.dim() == 4 and a.shape[0] == 1 and a.shape[1] == 3 and a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
        assert a.device == b.device, (a.device, b.device)
        H, W = int(a.shape[2]), int(a.shape[3])
        assert H >= 1 and W >= 1, (H, W)
        assert grid is None or (len(grid) == 2 and all(int(v) == v for v in grid)), grid
        Hs, Ws = (H, W) if grid is None else (int(grid[0]), int(grid[1]))
        assert Hs >= 1 and Ws >= 1 and Hs * Ws < 1 << 32, (Hs, Ws)
        return H, W, Hs, Ws

    def lightness_joint_hist(self, a, b, grid=None, out=None):
        """a (the decoded input), b (the enhanced frame): fp32 [1,3,H,W] -> uint32 [256,256] on the device: the number of samples
        of the `grid` = (Hs, Ws) (default: every pixel once; sample (i, j) is the pixel at row ((2i+1) H) // (2 Hs), column
        ((2j+1) W) // (2 Ws)) whose 8-bit lightness max(R, G, B) is x in `a` and y in `b`, at [x, y].  Nothing synchronises."""
        H, W, Hs, Ws = self._noref_args(a, b, grid)
        if out is None:
            out = torch.empty((256, 256), dtype=torch.uint32, device=a.device)
        assert tuple(out.shape) == (256, 256) and out.dtype == torch.uint32 and out.is_contiguous() and out.device == a.device
        self.lib.call("zt_lightness_joint_hist_f32", a, b, H, W, Hs, Ws, out, self._s(a))
        return out

    def noref(self, a, b, grid=None, out_i=None, out_f=None):
        """the no-reference numbers of frame `b` against its input `a` on `grid` (see `lightness_joint_hist`) -> (int64 [6],
        float64 [2]) on the device: {Ns, S_loe, S_a, S_b, n_sat, n_black} and the entropies in bits of the two lightness
        marginals (include/zerotig_hip.h).  Nothing synchronises; `out_i` / `out_f` (e.g. cells of a table row) are overwritten.
        The 256 KB histogram between the two kernels is cached per device."""
        self._noref_args(a, b, grid)
        dev = a.device
        ws = self.__dict__.setdefault("_noref_workspaces", {})
        if str(dev) not in ws:
            ws[str(dev)] = torch.empty((256, 256), dtype=torch.uint32, device=dev)
        if out_i is None:
            out_i = torch.empty(6, dtype=torch.int64, device=dev)
        if out_f is None:
            out_f = torch.empty(2, dtype=torch.float64, device=dev)
        assert tuple(out_i.shape) == (6,) and out_i.dtype == torch.int64 and out_i.is_contiguous() and out_i.device == dev
        assert tuple(out_f.shape) == (2,) and out_f.dtype == torch.float64 and out_f.is_contiguous() and out_f.device == dev
        hist = self.lightness_joint_hist(a, b, grid, out=ws[str(dev)])
        self.lib.call("zt_noref_from_hist", hist, out_i, out_f, self._s(a))
        return out_i, out_f

    # ---- no-reference colour grading of a frame (zt_color.hip) --------------------------------------------
    def color_stats(self, x, block=10, out_i=None, out_f=None, max_workgroups=0):
        """the raw numbers of UIQM, UCIQE and colourfulness of the fp32 [1,3,H,W] frame `x` with blocks of `block` x `block` pixels
        (4..64) -> (int64 [18], float64 [7]) on the device, as include/zerotig_hip.h lists them; `grading.color_values` turns them
        into the measures.  Nothing synchronises; `out_i` / `out_f` (e.g. cells of a table row) are overwritten.  `max_workgroups`
        caps the grid of the pass over the frame (0: the default).  The two CIELAB tables, made here in float64, and the
        workspace are cached per device."""
        import ctypes
        import numpy as np
        _f32c(x)
        assert x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 3, tuple(x.shape)
        H, W = int(x.shape[2]), int(x.shape[3])
        assert H >= 1 and W >= 1 and H * W < 1 << 31, (H, W)
        assert int(block) == block and 4 <= block <= 64, block
        assert int(max_workgroups) == max_workgroups and max_workgroups >= 0, max_workgroups
        dev = x.device
        cache = self.__dict__.setdefault("_color_cache", {})
        c = cache.get(str(dev))
        if c is None:
            v = np.arange(256, dtype=np.float64) / 255.0
            lin16 = np.rint(65535.0 * np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)).astype(np.int32)
            t = np.arange(65536, dtype=np.float64) / 65535.0
            flut = np.where(t > 216.0 / 24389.0, np.cbrt(t), (24389.0 / 27.0 * t + 16.0) / 116.0).astype(np.float32)
            c = cache[str(dev)] = {"lin16": torch.from_numpy(lin16).to(dev), "flut": torch.from_numpy(flut).to(dev), "ws": None}
        need = ctypes.c_size_t(0)
        self.lib.call("zt_color_ws_bytes", H, W, int(block), ctypes.byref(need))
        if c["ws"] is None or c["ws"].numel() * 8 < need.value:
            c["ws"] = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=dev)
        if out_i is None:
            out_i = torch.empty(18, dtype=torch.int64, device=dev)
        if out_f is None:
            out_f = torch.empty(7, dtype=torch.float64, device=dev)
        assert tuple(out_i.shape) == (18,) and out_i.dtype == torch.int64 and out_i.is_contiguous() and out_i.device == dev
        assert tuple(out_f.shape) == (7,) and out_f.dtype == torch.float64 and out_f.is_contiguous() and out_f.device == dev
        self.lib.call("zt_color_stats_f32", x, H, W, int(block), c["lin16"], c["flut"], int(max_workgroups), c["ws"],
                      c["ws"].numel() * 8, out_i, out_f, self._s(x))
        return out_i, out_f

    # ---- NIQE of a frame (zt_niqe.hip) --------------------------------------------------------------------
    def _niqe_cache(self, dev):
        """the Gaussian window and the three Gamma tables, made here in float64, and the buffers, per device"""
        from .grading import niqe_tables
        cache = self.__dict__.setdefault("_niqe_caches", {})
        c = cache.get(str(dev))
        if c is None:
            win, r_gam, c1, c2 = niqe_tables()
            c = cache[str(dev)] = {"win": torch.from_numpy(win).to(dev), "r_gam": torch.from_numpy(r_gam).to(dev),
                                   "c1": torch.from_numpy(c1).to(dev), "c2": torch.from_numpy(c2).to(dev), "ws": None, "sums": {}}
        return c

    def niqe_block_sums(self, x, max_workgroups=0, out_i=None, out_f=None):
        """the block sums of NIQE of the fp32 [1,3,H,W] frame `x` (H, W >= 96), both scales -> (int64 [2,nblk,10], float64
        [2,nblk,16]) on the device, as include/zerotig_hip.h lists them; nblk = (H // 96) * (W // 96).  Nothing synchronises.
        `max_workgroups` caps the grid of the tile pass (0: no cap); the sums do not depend on it."""
        import ctypes
        _f32c(x)
        assert x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 3, tuple(x.shape)
        H, W = int(x.shape[2]), int(x.shape[3])
        assert H >= 96 and W >= 96 and H * W < 1 << 31, (H, W)
        assert int(max_workgroups) == max_workgroups and max_workgroups >= 0, max_workgroups
        dev, nblk = x.device, (H // 96) * (W // 96)
        c = self._niqe_cache(dev)
        need = ctypes.c_size_t(0)
        self.lib.call("zt_niqe_ws_bytes", H, W, ctypes.byref(need))
        if c["ws"] is None or c["ws"].numel() * 8 < need.value:
            c["ws"] = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=dev)
        if out_i is None:
            out_i = torch.empty((2, nblk, 10), dtype=torch.int64, device=dev)
        if out_f is None:
            out_f = torch.empty((2, nblk, 16), dtype=torch.float64, device=dev)
        assert tuple(out_i.shape) == (2, nblk, 10) and out_i.dtype == torch.int64 and out_i.is_contiguous() and out_i.device == dev
        assert tuple(out_f.shape) == (2, nblk, 16) and out_f.dtype == torch.float64 and out_f.is_contiguous() and out_f.device == dev
        self.lib.call("zt_niqe_block_sums_f32", x, H, W, c["win"], int(max_workgroups), c["ws"], c["ws"].numel() * 8, out_i, out_f,
                      self._s(x))
        return out_i, out_f

    def niqe_frame_from_sums(self, sums_i, sums_f, out_i=None, out_f=None):
        """the ten fits of every block and the frame's reduction from what `niqe_block_sums` returns (or the same of any rows of
        it, [2,n,10] / [2,n,16]) -> (int64 [38], float64 [738]) on the device; `grading.niqe_value` turns them into the score"""
        dev = sums_i.device
        nblk = int(sums_i.shape[1])
        assert nblk >= 1 and tuple(sums_i.shape) == (2, nblk, 10) and sums_i.dtype == torch.int64 and sums_i.is_contiguous()
        assert tuple(sums_f.shape) == (2, nblk, 16) and sums_f.dtype == torch.float64 and sums_f.is_contiguous() and sums_f.device == dev
        c = self._niqe_cache(dev)
        if out_i is None:
            out_i = torch.empty(38, dtype=torch.int64, device=dev)
        if out_f is None:
            out_f = torch.empty(738, dtype=torch.float64, device=dev)
        assert tuple(out_i.shape) == (38,) and out_i.dtype == torch.int64 and out_i.is_contiguous() and out_i.device == dev
        assert tuple(out_f.shape) == (738,) and out_f.dtype == torch.float64 and out_f.is_contiguous() and out_f.device == dev
        self.lib.call("zt_niqe_frame_f32", sums_i, sums_f, nblk, c["r_gam"], c["c1"], c["c2"], out_i, out_f, self._s(sums_i))
        return out_i, out_f

    def niqe_frame(self, x, out_i=None, out_f=None):
        """the raw numbers of NIQE of the fp32 [1,3,H,W] frame `x` (H, W >= 96) -> (int64 [38], float64 [738]) on the device:
        {nblk, valid rows, count per column}, {column sums, mean of the valid rows, their centred scatter}.  Nothing synchronises;
        `out_i` / `out_f` (e.g. cells of a table row) are overwritten.  The block sums between the two kernels, the tables and the
        workspace are cached per device."""
        H, W = int(x.shape[2]), int(x.shape[3])
        nblk = (H // 96) * (W // 96)
        assert nblk >= 1, (H, W)
        c = self._niqe_cache(x.device)
        if nblk not in c["sums"]:
            c["sums"][nblk] = (torch.empty((2, nblk, 10), dtype=torch.int64, device=x.device),
                               torch.empty((2, nblk, 16), dtype=torch.float64, device=x.device))
        si, sf = self.niqe_block_sums(x, out_i=c["sums"][nblk][0], out_f=c["sums"][nblk][1])
        return self.niqe_frame_from_sums(si, sf, out_i, out_f)

    def psnr_u8(self, a, b):
        """evals.py:83-85: cv2.PSNR of round(a*255), round(b*255) -> python float (inf when identical); one 8-byte read-back."""
        _f32c(a), _f32c(b)
        n = a.numel()
        assert b.numel() == n
        nblk = max(1, min(1024, n // 4096))
        part = torch.empty(nblk, dtype=torch.int64, device=a.device)
        out = torch.empty(1, dtype=torch.int64, device=a.device)
        self.lib.call("zt_sqdiff_u8_f32", a, b, n, part, nblk, out, self._s(a))
        import math
        sq = int(out.item())
        return float("inf") if sq == 0 else 10.0 * math.log10(255.0 ** 2 * n / sq)

    def ssim_u8(self, a, b):
        """evals.py:87: skimage structural_similarity(round(a*255), round(b*255), channel_axis=2, data_range=255) of two
        [1,3,H,W] frames -> python float; fp64 on the device, one 8-byte read-back."""
        _f32c(a), _f32c(b)
        assert a.dim() == 4 and a.shape[0] == 1 and a.shape[1] == 3 and a.shape == b.shape, (a.shape, b.shape)
        H, W = int(a.shape[2]), int(a.shape[3])
        npart = 3 * max(1, -(-(H - 6) // 32)) * max(1, -(-(W - 6) // 64))
        part = torch.empty(npart, dtype=torch.float64, device=a.device)
        out = torch.empty(1, dtype=torch.float64, device=a.device)
        self.lib.call("zt_ssim_u8_f32", a, b, H, W, part, npart, out, self._s(a))
        return float(out.item())

    def match_histograms(self, src, tmpl):
        """evals.py:100-103: skimage exposure.match_histograms(src, tmpl), all channels pooled (its channel_axis=None default)
        -> fp32 tensor of src's shape on the device.  tmpl is a ToTensor image (values k/255) of any size."""
        _f32c(src), _f32c(tmpl)
        n, m = src.numel(), tmpl.numel()
        out = torch.empty_like(src)
        nbytes = 8 * ((n + 3) & ~3) + 1024 * (-(-n // 4096)) + 8192
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
        self.lib.call("zt_match_histograms_f32", src, n, tmpl, m, out, scratch, nbytes, self._s(src))
        return out

    # ---- LPIPS (zt_lpips.hip) -----------------------------------------------------------------------------------
    def lpips_prep(self, img, dtype=torch.float32):
        """[1,3,H,W] fp32 in [0,1] -> nhwc [1,H,W,8] (fp32 or bf16): (img - 0.5) * 2 through lpips' scaling layer; channels 3..7 zero."""
        _f32c(img)
        assert img.dim() == 4 and img.shape[0] == 1 and img.shape[1] == 3, img.shape
        H, W = int(img.shape[2]), int(img.shape[3])
        out = torch.empty((1, H, W, 8), dtype=dtype, device=img.device)
        self.lib.call("zt_lpips_prep", img, out, _dt(out), H, W, self._s(img))
        return out

    def maxpool2(self, x):
        """nn.MaxPool2d(2, 2) of a CV/tensor NHWC (fp32 or bf16) -> [N, H // 2, W // 2, C]"""
        x = _cv(x)
        out = torch.empty((x.N, x.H // 2, x.W // 2, x.C), dtype=x.t.dtype, device=x.t.device)
        self.lib.call("zt_maxpool2_nhwc", x.ptr, _dt(x.t), x.ld, x.N, x.H, x.W, x.C, out, x.C, self._s(x.t))
        return out

    def conv3x3_wide_bf16(self, x, wdev, bias, Cout, relu=True, out=None):
        """y = [relu](conv3x3(x) + bias), pad 1, for Cin % 64 == 0 and Cout % 128 == 0: bf16 NHWC in and out, wdev bf16 [9, CoutP, ldk]."""
        x = _cv(x)
        assert x.t.dtype == torch.bfloat16 and wdev.dtype == torch.bfloat16 and wdev.shape[0] == 9
        if out is None:
            out = torch.empty((x.N, x.H, x.W, Cout), dtype=torch.bfloat16, device=x.t.device)
        o = _cv(out)
        assert o.t.dtype == torch.bfloat16 and (o.N, o.H, o.W) == (x.N, x.H, x.W)
        tok = self._ev_begin(self.profile["match"].get((3, 3, 1, x.C, Cout, x.H, x.W))) if self.profile else None
        self.lib.call("zt_conv3x3_wide_bf16", x.ptr, x.ld, x.N, x.H, x.W, x.C, wdev, wdev.shape[1], wdev.shape[2], bias, o.ptr, o.ld,
                      Cout, int(relu), self._s(x.t))
        self._ev_end(tok)
        return out

    def lpips_layer(self, fa, fb, w, out):
        """out[0] (fp64, device) = one tap's LPIPS term of two NHWC feature maps (N == 1, same dtype); w: fp32 [C] lin weights."""
        fa, fb = _cv(fa), _cv(fb)
        assert fa.t.dtype == fb.t.dtype and (fa.N, fa.H, fa.W, fa.C) == (fb.N, fb.H, fb.W, fb.C) and fa.N == 1
        assert w.dtype == torch.float32 and w.numel() == fa.C and out.dtype == torch.float64
        part = torch.empty(2048, dtype=torch.float64, device=fa.t.device)
        self.lib.call("zt_lpips_layer", fa.ptr, fa.ld, fb.ptr, fb.ld, _dt(fa.t), fa.H * fa.W, fa.C, w, part, 2048, out, self._s(fa.t))

    # ---- convolution family (zt_conv*.hip, zt_wgrad.hip) ------------------------------------------------
    def repack_weight(self, w, ldw=None, co_off=0, transpose_flip=False, out=None):
        """torch [Cout,Cin,KH,KW] -> device layout [KH*KW, Cin', ldw]."""
        _f32c(w)
        Cout, Cin, KH, KW = w.shape
        n_out, n_in = (Cin, Cout) if transpose_flip else (Cout, Cin)
        if ldw is None:
            ldw = (n_out + 15) // 16 * 16
        if out is None:
            out = torch.zeros((KH * KW, n_in, ldw), dtype=torch.float32, device=w.device)
        self.lib.call("zt_repack_conv_weight_f32", w, out, Cout, Cin, KH, KW, ldw, co_off, int(transpose_flip), self._s(w))
        return out

    def conv2d(self, x, wdev, bias, Cout, KH, KW, stride=1, pad=(0, 0), act=None, alpha=1.0, x2=None, out=None,
               out_planar=False, aux=None, epi=0, w_coff=0, out2=None, esplit=0):
        """x: CV/tensor NHWC; optional x2 (CV) supplies channels >= x.C.  out: CV (nhwc) or planar tensor [N,Cout,Ho,Wo]."""
        x = _cv(x)
        Cin, csplit, ldx2, x2p = x.C, 0, 0, None
        if x2 is not None:
            x2 = _cv(x2)
            csplit, Cin, ldx2, x2p = x.C, x.C + x2.C, x2.ld, x2.ptr
        assert wdev.shape[1] == Cin and wdev.shape[0] == KH * KW, (wdev.shape, Cin, KH, KW)
        ldw = wdev.shape[2]
        Ho = (x.H + 2 * pad[0] - KH) // stride + 1
        Wo = (x.W + 2 * pad[1] - KW) // stride + 1
        dev = x.t.device
        if out_planar:
            if out is None:
                out = torch.empty((x.N, Cout, Ho, Wo), dtype=torch.float32, device=dev)
            yptr, ldy = out.data_ptr(), out.stride(1)
        else:
            if out is None:
                out = torch.empty((x.N, Ho, Wo, (Cout + 3) // 4 * 4), dtype=torch.float32, device=dev)
                if out.shape[-1] != Cout:
                    out.zero_()
            o = _cv(out)
            assert (o.N, o.H, o.W) == (x.N, Ho, Wo) and o.C >= Cout
            yptr, ldy = o.ptr, o.ld
        auxp, ldaux = None, 0
        if epi:
            av = _cv(aux)
            auxp, ldaux = av.ptr, av.ld
        tok = self._ev_begin(self.profile["match"].get((KH, KW, stride, Cin, Cout, x.H, x.W))) if self.profile else None
        if epi >= 4:            # fused SepConvGRU epilogues
            o2 = _cv(out2) if out2 is not None else None
            self.lib.call("zt_conv2d_nhwc_f32_ex", x.ptr, x2p, csplit, x.ld, ldx2, x.N, x.H, x.W, Cin, wdev.data_ptr() + 4 * w_coff, ldw, bias,
                          yptr, ldy, int(out_planar), Cout, KH, KW, stride, pad[0], pad[1], ACT[act], float(alpha), auxp, ldaux, epi,
                          o2.ptr if o2 else None, o2.ld if o2 else 0, esplit, self._s(x.t))
        else:
            self.lib.call("zt_conv2d_nhwc_f32", x.ptr, x2p, csplit, x.ld, ldx2, x.N, x.H, x.W, Cin, wdev.data_ptr() + 4 * w_coff, ldw, bias,
                          yptr, ldy, int(out_planar), Cout, KH, KW, stride, pad[0], pad[1], ACT[act], float(alpha), auxp, ldaux, epi,
                          self._s(x.t))
        self._ev_end(tok)
        return out

    def slab(self, dev, nbytes=96 << 20):
        key = (dev, nbytes)
        if key not in self._slab:
            self._slab[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        return self._slab[key]

    def conv2d_wgrad(self, x, dz, Cout, KH, KW, grad_w, accumulate=False, slab=None, grad_b=None):
        """grad_w [Cout,Cin,KH,KW] (+)= wgrad of a stride-1 same conv; x, dz: CV/tensor NHWC (N == 1)."""
        x, dz = _cv(x), _cv(dz)
        assert x.N == 1 and (x.H, x.W) == (dz.H, dz.W) and dz.C >= Cout
        assert tuple(grad_w.shape) == (Cout, x.C, KH, KW) and grad_w.is_contiguous()
        slab = self.slab(x.t.device) if slab is None else slab
        self.lib.call("zt_conv2d_wgrad_nhwc_f32", x.ptr, x.ld, dz.ptr, dz.ld, x.H, x.W, x.C, Cout, KH, KW, slab,
                      slab.numel() * 4, grad_w, grad_b, int(accumulate), self._s(x.t))
        return grad_w

    # ---- normalisation (zt_norm.hip) --------------------------------------------------------------------------
    def _nblk(self, HW):
        # one partial row per workgroup; 256 = one workgroup per CU.  More rows only lengthen the finalize kernel's serial sum
        # (10 us with 900 rows on the 180 x 320 RAFT maps, 4 us with 256) without making the statistics pass any faster.
        return max(1, min(256 if HW < (1 << 20) else _NBLK_BIG, HW // 64))

    def chan_stats(self, x, nblk=None):
        """-> partial [N, nblk, 2, C] (sum, sum of squares) for a CV/tensor NHWC."""
        x = _cv(x)
        HW = x.H * x.W
        nblk = self._nblk(HW) if nblk is None else nblk
        part = torch.empty((x.N, nblk, 2, x.C), dtype=torch.float32, device=x.t.device)
        self.lib.call("zt_chan_stats_nhwc", x.ptr, _dt(x.t), x.ld, x.N, HW, x.C, nblk, part, self._s(x.t))
        return part

    def instance_norm_stats(self, x, eps=1e-5):
        """InstanceNorm scale/shift [N, C] of a CV/tensor NHWC in one launch: the statistics kernel's last workgroup per sample
        does the finalize (zt_norm.hip instnorm_tail).  Ticket counters come from a zero-initialised pool and return to zero."""
        x = _cv(x)
        HW = x.H * x.W
        nblk = self._nblk(HW)
        dev = x.t.device
        pool = self._tickets.get(dev)
        if pool is None:
            pool = self._tickets[dev] = [torch.zeros(4096, dtype=torch.int32, device=dev), 0]
        if pool[1] + x.N > 4096:
            pool[1] = 0
        tick = pool[0][pool[1]:pool[1] + x.N]
        pool[1] += x.N
        part = torch.empty((x.N, nblk, 2, x.C), dtype=torch.float32, device=dev)
        scale = torch.empty((x.N, x.C), dtype=torch.float32, device=dev)
        shift = torch.empty_like(scale)
        self.lib.call("zt_instance_norm_stats", x.ptr, _dt(x.t), x.ld, x.N, HW, x.C, nblk, part, float(eps), tick, scale, shift,
                      self._s(x.t))
        return scale, shift

    def norm_finalize(self, part, N, C, count, mode, gamma=None, beta=None, rm=None, rv=None, nbt=None, momentum=0.1,
                      eps=1e-5, dev=None):
        dev = part.device if part is not None else dev
        scale = torch.empty((N, C), dtype=torch.float32, device=dev)
        shift, mean, rstd = torch.empty_like(scale), torch.empty_like(scale), torch.empty_like(scale)
        nblk = part.shape[1] if part is not None else 0
        self.lib.call("zt_norm_finalize_f32", part, nblk, N, C, count, eps, mode, gamma, beta, rm, rv, nbt, momentum,
                      scale, shift, mean, rstd, current_stream(dev))
        return scale, shift, mean, rstd

    def norm_apply(self, x, scale, shift, out=None, res=None, inner_relu=False, outer_relu=False):
        x = _cv(x)
        if out is None:
            out = torch.empty((x.N, x.H, x.W, x.C), dtype=x.t.dtype, device=x.t.device)
        o = _cv(out)
        rp, ldr = (None, 0) if res is None else (_cv(res).ptr, _cv(res).ld)
        assert o.t.dtype == x.t.dtype and (res is None or _cv(res).t.dtype == x.t.dtype)
        self.lib.call("zt_norm_apply_nhwc", x.ptr, _dt(x.t), x.ld, scale, shift, rp, ldr, o.ptr, o.ld, x.N, x.H * x.W, x.C,
                      int(inner_relu), int(outer_relu), self._s(x.t))
        return out

    def loss_terms_reduce(self, p1, nb1, p2, nb2, p3, nb3, terms):
        """terms[0:17] from the three partial buffers of the loss kernels (one launch for five partial_reduce calls)"""
        self.lib.call("zt_loss_terms_reduce_f32", p1, nb1, p2, nb2, p3, nb3, terms, self._s(p1))
        return terms

    def partial_reduce(self, part, nblk, stride, n, out=None, accumulate=False, out2=None):
        self.lib.call("zt_partial_reduce_f32", part, nblk, stride, n, out, int(accumulate), out2, self._s(part))

    def bn_relu_bwd(self, dy, z, scale, shift, mean, rstd, dgamma, dbeta, out=None, eval_mode=False, part=None):
        """backward of ReLU(BN(z)) for N == 1 (train-mode batch statistics, or eval_mode: running statistics are constants);
        accumulates dgamma/dbeta; returns dz (NHWC).  part: the reduce pass's partials as produced by the data-gradient kernel that
        wrote dy (`conv3x3_dgrad_bn_sums_bf16`: [nblk][2][C] = (sum g, sum g (z - mean))) -- the separate reduce launch is skipped."""
        dy, z = _cv(dy), _cv(z)
        HW, C = z.H * z.W, z.C
        assert dy.t.dtype == z.t.dtype
        sums = torch.empty((2, C), dtype=torch.float32, device=z.t.device)
        if part is not None:
            self.lib.call("zt_bn_bwd_sums_centered_f32", part, part.shape[0], C, rstd, dbeta, dgamma, sums, self._s(z.t))
        else:
            nblk = self._nblk(HW)
            part = torch.empty((nblk, 2, C), dtype=torch.float32, device=z.t.device)
            self.lib.call("zt_bn_bwd_reduce", dy.ptr, _dt(z.t), dy.ld, z.ptr, z.ld, scale, shift, mean, rstd, HW, C, nblk, part, self._s(z.t))
            self.lib.call("zt_bn_bwd_sums_f32", part, nblk, C, dbeta, dgamma, sums, self._s(z.t))
        if out is None:
            out = torch.empty((1, z.H, z.W, C), dtype=z.t.dtype, device=z.t.device)
        o = _cv(out)
        self.lib.call("zt_bn_bwd_apply", dy.ptr, _dt(z.t), dy.ld, z.ptr, z.ld, scale, shift, mean, rstd, sums, o.ptr, o.ld, HW, C,
                      int(eval_mode), self._s(z.t))
        return out

    # ---- RAFT specific (zt_raft.hip) --------------------------------------------------------------------------
    def resize_bilinear(self, x, h, w, mul=1.0):
        _, C, H, W = x.shape
        out = torch.empty((1, C, h, w), dtype=torch.float32, device=x.device)
        self.lib.call("zt_resize_bilinear_f32", x, out, C, H, W, h, w, float(mul), self._s(x))
        return out

    def equalize_prepare(self, x255):
        """x255: [1,C,h,w] float in [0,255] -> (uint8 truncation [C,hw], hist int32 [C,256], lut int32 [C,256])."""
        _, C, h, w = x255.shape
        q = torch.empty((C, h * w), dtype=torch.uint8, device=x255.device)
        hist = torch.empty((C, 256), dtype=torch.int32, device=x255.device)
        lut = torch.empty((C, 256), dtype=torch.int32, device=x255.device)
        self.lib.call("zt_equalize_prepare_u8", x255, q, hist, lut, C, h * w, self._s(x255))
        return q, hist, lut

    def raft_pack_input(self, img1, q2, lut, h, w, dtype=torch.float32):
        Hp, Wp = (h + 7) // 8 * 8, (w + 7) // 8 * 8
        ld = 8 if dtype == torch.bfloat16 else 4
        out = torch.empty((2, Hp, Wp, ld), dtype=dtype, device=img1.device)
        self.lib.call("zt_raft_pack_input", img1, q2, lut, out, _dt(out), ld, h, w, Hp, Wp, self._s(img1))
        return out

    def raft_stem_weight_bf16(self, w):
        """torch [64,3,7,7] fp32 -> [7,64,64] bf16 (k = kx*8 + c) for raft_stem_bf16"""
        _f32c(w)
        assert tuple(w.shape) == (64, 3, 7, 7)
        out = torch.empty((7, 64, 64), dtype=torch.bfloat16, device=w.device)
        self.lib.call("zt_repack_stem_weight_bf16", w, out, self._s(w))
        return out

    def raft_stem_bf16(self, x, wstem, bias, relu=False):
        """x: nhwc [N,H,W,8] bf16 (channels 3..7 zero) -> conv7x7 s2 p3 + bias (+ ReLU): nhwc [N,H/2,W/2,64] bf16 (extractor.py:120)"""
        assert x.dtype == torch.bfloat16 and x.shape[-1] == 8 and x.is_contiguous()
        N, H, W, _ = x.shape
        out = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), dtype=torch.bfloat16, device=x.device)
        self.lib.call("zt_raft_stem_conv_bf16", x, N, H, W, wstem, bias, out, 64, int(relu), self._s(x))
        return out

    def corr_pyramid(self, corr0, h, w):
        """corr0: NHWC [1,h,w,ld>=h*w] level 0 -> [level1, level2, level3] tensors [npx, hl, wl]."""
        npx = h * w
        levels, src, hin, win, ldin = [], corr0, h, w, corr0.shape[-1]
        for hl, wl in _pooled_dims(h, w):
            dst = torch.empty((npx, hl, wl), dtype=torch.float32, device=corr0.device)
            self.lib.call("zt_corr_pool_f32", src, dst, npx, hin, win, ldin, self._s(corr0))
            levels.append(dst)
            src, hin, win, ldin = dst, hl, wl, hl * wl
        return levels

    def corr_volume_pyramid_bf16(self, fmap1, fmap2, h, w, alpha):
        """fmap1 / fmap2: bf16 [.., 256]-channel NHWC feature maps of the two frames ([npx][ld] views) -> (corr0 [1,h,w,ld0] fp32,
        [level1, level2, level3]) in one launch (corr.py:13-27, 52-60).  ld0 = npx rounded up to 4; the launch does not write the
        padding columns npx .. ld0 - 1 of corr0, which keep whatever the allocation held (the lookup never reads them)."""
        npx = h * w
        ld0 = (npx + 3) // 4 * 4
        dev = fmap1.device
        corr0 = torch.empty((1, h, w, ld0), dtype=torch.float32, device=dev)
        levels = [torch.empty((npx, a, b), dtype=torch.float32, device=dev) for a, b in _pooled_dims(h, w)]
        tok = self._ev_begin(self.profile["match"].get((1, 1, 1, 256, npx, h, w))) if self.profile else None
        self.lib.call("zt_corr_volume_pyramid_bf16", fmap1, fmap1.shape[-1], fmap2, fmap2.shape[-1], h, w, float(alpha), corr0, ld0,
                      levels[0], levels[1], levels[2], self._s(fmap1))
        self._ev_end(tok)
        return corr0, levels

    def _lookup(self, name, head, out, book, stream):
        """one launch of the lookup entry point `name`; with a book = (delta, coords_out, f4, fhx_ptr, ldfhx, fin), of its _step form:
        the lookup at coords + delta with the previous iteration's flow bookkeeping folded in (ZtFlowBook, zt_lookup.h)."""
        if book is not None:
            delta, coords_out, f4, fhx_ptr, ldfhx, fin = book
            name += "_step"
            head += (delta, 0 if delta is None else delta.shape[-1], coords_out, f4, f4.shape[-1], fhx_ptr, ldfhx, fin, fin.shape[-1])
        self.lib.call(name, *head, stream)
        return out

    def corr_lookup(self, corr0, levels, h, w, coords, out=None, book=None):
        if out is None:
            out = torch.empty((1, h, w, 324), dtype=torch.float32, device=corr0.device)
        head = (corr0, levels[0], levels[1], levels[2], h, w, corr0.shape[-1], coords, out, _dt(out), out.shape[-1], h * w)
        return self._lookup("zt_corr_lookup", head, out, book, self._s(corr0))

    def corr_lookup_step(self, corr0, levels, h, w, coords, out, delta, coords_out, f4, fhx_ptr, ldfhx, fin):
        """lookup at coords + delta with the previous iteration's flow bookkeeping folded in (zt_corr_lookup_step)."""
        return self.corr_lookup(corr0, levels, h, w, coords, out, book=(delta, coords_out, f4, fhx_ptr, ldfhx, fin))

    # ---- on-the-fly correlation (zt_corr_alt.hip): the same lookup from the feature maps, no volume -----------------
    def fmap_pyramid(self, fmap2, h, w):
        """fmap2: nhwc [>= h*w rows][ld >= 256] (fp32 or bf16, 256 channels) -> [P1, P2, P3] fp32 [hl*wl, 256], avg_pool2d(2, 2)
        with floor sizes, each level from the rounded level below."""
        f2 = fmap2.view(-1, fmap2.shape[-1])
        assert f2.shape[0] >= h * w and f2.is_contiguous()
        lv = [torch.empty((a * b, 256), dtype=torch.float32, device=fmap2.device) for a, b in _pooled_dims(h, w)]
        self.lib.call("zt_fmap_pyramid", f2, _dt(f2), f2.shape[-1], h, w, lv[0], lv[1], lv[2], self._s(fmap2))
        return lv

    def corr_alt_lookup(self, fmap1, fmap2, pyr, h, w, coords, out=None, alpha=1.0 / 16.0, book=None):
        """corr_lookup's output computed from fmap1 / fmap2 ([npx][ld] nhwc views of one storage type) and fmap_pyramid(fmap2)."""
        if out is None:
            out = torch.empty((1, h, w, 324), dtype=torch.float32, device=fmap1.device)
        assert fmap1.dtype == fmap2.dtype
        head = (fmap1, fmap1.shape[-1], fmap2, fmap2.shape[-1], _dt(fmap1), pyr[0], pyr[1], pyr[2], h, w, float(alpha), coords, out,
                _dt(out), out.shape[-1], h * w)
        return self._lookup("zt_corr_alt_lookup", head, out, book, self._s(fmap1))

    def corr_alt_lookup_step(self, fmap1, fmap2, pyr, h, w, coords, out, delta, coords_out, f4, fhx_ptr, ldfhx, fin, alpha=1.0 / 16.0):
        """corr_alt_lookup at coords + delta with the previous iteration's flow bookkeeping folded in, as corr_lookup_step."""
        return self.corr_alt_lookup(fmap1, fmap2, pyr, h, w, coords, out, alpha, book=(delta, coords_out, f4, fhx_ptr, ldfhx, fin))

    # ---- bf16 throughput mode of the convolution family ---------------------------------------------------------
    def repack_weight_bf16(self, w, transpose_flip=False, out=None, co_off=0):
        """torch fp32 [Cout,Cin,KH,KW] -> bf16 [KH*KW, CoutP16, ldk8] (input channel fastest); zero padded."""
        _f32c(w)
        Cout, Cin, KH, KW = w.shape
        n_out, n_in = (Cin, Cout) if transpose_flip else (Cout, Cin)
        if out is None:
            CoutP, ldk = (n_out + 15) // 16 * 16, (n_in + 7) // 8 * 8
            out = torch.zeros((KH * KW, CoutP, ldk), dtype=torch.bfloat16, device=w.device)
        CoutP, ldk = out.shape[1], out.shape[2]
        self.lib.call("zt_repack_conv_weight_bf16", w, out, Cout, Cin, KH, KW, CoutP, ldk, co_off, int(transpose_flip), self._s(w))
        return out

    def conv2d_bf16(self, x, wdev, bias, Cout, KH, KW, pad=(0, 0), act=None, alpha=1.0, out=None, out_planar=False, aux=None, epi=0,
                    stride=1, x2=None, out_f32=False, w_roff=0, variant=0, out2=None, esplit=0):
        """x (and optional x2 for channels >= x.C): CV over bf16 NHWC buffers.  out: bf16 NHWC (default), fp32 NHWC (out_f32)
        or fp32 planar [N,Cout,Ho,Wo] (out_planar).  w_roff: first output-channel row of wdev to use."""
        x = _cv(x)
        assert x.t.dtype == torch.bfloat16 and wdev.dtype == torch.bfloat16 and wdev.shape[0] == KH * KW
        Cin, csplit, ldx2, x2p = x.C, 0, 0, None
        if x2 is not None:
            x2 = _cv(x2)
            assert x2.t.dtype == torch.bfloat16
            csplit, Cin, ldx2, x2p = x.C, x.C + x2.C, x2.ld, x2.ptr
        CoutP, ldk = wdev.shape[1] - w_roff, wdev.shape[2]
        assert ldk >= Cin and CoutP >= Cout and (KH * KW == 1 or w_roff == 0)
        Ho = (x.H + 2 * pad[0] - KH) // stride + 1
        Wo = (x.W + 2 * pad[1] - KW) // stride + 1
        dev = x.t.device
        if out_planar:
            if out is None:
                out = torch.empty((x.N, Cout, Ho, Wo), dtype=torch.float32, device=dev)
            yptr, ldy, mode = out.data_ptr(), out.stride(1), 1
        else:
            odt = torch.float32 if out_f32 else torch.bfloat16
            gran = 4 if out_f32 else 8
            if out is None:
                ld = (Cout + gran - 1) // gran * gran
                out = torch.empty((x.N, Ho, Wo, ld), dtype=odt, device=dev)
                if ld != Cout:
                    out.zero_()
            o = _cv(out)
            assert o.t.dtype == odt and (o.N, o.H, o.W) == (x.N, Ho, Wo) and o.C >= Cout
            yptr, ldy, mode = o.ptr, o.ld, (2 if out_f32 else 0)
        auxp, ldaux = None, 0
        if epi:
            av = _cv(aux)
            assert av.t.dtype == torch.bfloat16
            auxp, ldaux = av.ptr, av.ld
        tok = self._ev_begin(self.profile["match"].get((KH, KW, stride, Cin, Cout, x.H, x.W))) if self.profile else None
        if epi >= 4:            # fused SepConvGRU epilogues (4, 5); ResidualBlock tail relu(act(conv) + aux) (6)
            o2 = _cv(out2) if out2 is not None else None
            assert o2 is None or o2.t.dtype == torch.bfloat16
            self.lib.call("zt_conv2d_nhwc_bf16_ex", x.ptr, x2p, csplit, x.ld, ldx2, x.N, x.H, x.W, Cin,
                          wdev.data_ptr() + 2 * w_roff * ldk, CoutP, ldk, bias, yptr, ldy, mode, Cout, KH, KW, stride, pad[0], pad[1],
                          ACT[act], float(alpha), auxp, ldaux, epi, o2.ptr if o2 else None, o2.ld if o2 else 0, esplit, self._s(x.t))
            self._ev_end(tok)
            return out
        self.lib.call("zt_conv2d_nhwc_bf16_variant", x.ptr, x2p, csplit, x.ld, ldx2, x.N, x.H, x.W, Cin,
                      wdev.data_ptr() + 2 * w_roff * ldk, CoutP, ldk, bias, yptr, ldy, mode, Cout, KH, KW, stride, pad[0], pad[1],
                      ACT[act], float(alpha), auxp, ldaux, epi, variant, self._s(x.t))
        self._ev_end(tok)
        return out

    def denoise_fused_bf16(self, srcs, refs, w1, b1, w2, b2, w3, b3, cout, out=None, want_res=False):
        """Whole Denoise_1 / Denoise_2 forward + tail in one launch (zt_denoise_fused_bf16): srcs = 1 or 4 planar fp32 [1,3,H,W]
        tensors (concatenated), refs = the planar fp32 tensors subtracted from ([x] or [H2, s2]); w1/w2/w3 bf16 device layouts
        [9,48,8|16] / [9,48,48] / [1,16,48], fp32 biases.  -> out [1,cout,H,W] = clamp(cat(refs) - net(cat(srcs)), 1e-4, 1)
        (and the residual net(cat(srcs)) when want_res)."""
        assert len(srcs) in (1, 4) and len(refs) * 3 == cout and cout in (3, 6)
        for t in list(srcs) + list(refs):
            _f32c(t)
            assert tuple(t.shape) == tuple(srcs[0].shape) and t.shape[0] == 1 and t.shape[1] == 3
        assert w1.dtype == w2.dtype == w3.dtype == torch.bfloat16
        assert tuple(w1.shape[:2]) == (9, 48) and w1.shape[2] in (8, 16) and w1.shape[2] >= 3 * len(srcs)
        assert tuple(w2.shape) == (9, 48, 48) and tuple(w3.shape) == (1, 16, 48)
        _, _, H, W = srcs[0].shape
        dev = srcs[0].device
        if out is None:
            out = torch.empty((1, cout, H, W), dtype=torch.float32, device=dev)
        assert tuple(out.shape) == (1, cout, H, W) and out.dtype == torch.float32 and out.is_contiguous()
        res = torch.empty_like(out) if want_res else None
        s = list(srcs) + [None] * (4 - len(srcs))
        self.lib.call("zt_denoise_fused_bf16", s[0], s[1], s[2], s[3], len(srcs), refs[0], refs[1] if cout == 6 else None,
                      w1, w1.shape[2], _f32c(b1), w2, _f32c(b2), w3, _f32c(b3), cout, out, res, H, W, self._s(out))
        return (out, res) if want_res else out

    def conv_pair_bf16(self, xA, wA, bA, CoutA, KA, outA, xB, wB, bB, CoutB, KB, outB, act=None):
        """Two independent stride-1 'same' convolutions (square kernels KA / KB) over the same map in ONE launch
        (zt_conv2d_pair_nhwc_bf16): bf16 NHWC in and out, y = act(conv + bias)."""
        xA, xB, oA, oB = _cv(xA), _cv(xB), _cv(outA), _cv(outB)
        assert (xA.N, xA.H, xA.W) == (xB.N, xB.H, xB.W) == (oA.N, oA.H, oA.W) == (oB.N, oB.H, oB.W)
        assert all(t.t.dtype == torch.bfloat16 for t in (xA, xB, oA, oB)) and wA.shape[0] == KA * KA and wB.shape[0] == KB * KB
        assert wA.shape[2] >= xA.C and wB.shape[2] >= xB.C and wA.shape[1] >= CoutA and wB.shape[1] >= CoutB and oA.C >= CoutA and oB.C >= CoutB
        self.lib.call("zt_conv2d_pair_nhwc_bf16", xA.ptr, xA.ld, xA.C, wA, wA.shape[1], wA.shape[2], bA, oA.ptr, oA.ld, CoutA, KA,
                      xB.ptr, xB.ld, xB.C, wB, wB.shape[1], wB.shape[2], bB, oB.ptr, oB.ld, CoutB, KB, xA.N, xA.H, xA.W, ACT[act], self._s(xA.t))

    # ---- deferred, batched weight gradients / weight repacks (bf16 mode) -----------------------------------------------
    def wgrad_partial_bf16(self, x, dz, Cout, K, slab, slab_off, relu_mask=None):
        """Append the per-workgroup slabs of one weight-gradient call to `slab` (fp32 tensor) at float offset slab_off.
        -> number of slabs written."""
        import ctypes
        x, dz = _cv(x), _cv(dz)
        assert x.t.dtype == torch.bfloat16 and dz.t.dtype == torch.bfloat16 and x.N == 1 and (x.H, x.W) == (dz.H, dz.W) and dz.C >= Cout
        mk = _cv(relu_mask) if relu_mask is not None else None
        n = ctypes.c_int(0)
        tok = self._ev_begin(self.profile["match"].get(("wgrad", K, x.C, Cout, x.H, x.W))) if self.profile else None
        self.lib.call("zt_conv2d_wgrad_partial_bf16", x.ptr, x.ld, dz.ptr, dz.ld, x.H, x.W, x.C, Cout, K, K, slab.data_ptr() + 4 * slab_off,
                      (slab.numel() - slab_off) * 4, mk.ptr if mk else None, mk.ld if mk else 0, ctypes.byref(n), self._s(x.t))
        self._ev_end(tok)
        return n.value

    def thin1x1_bwd_bf16(self, dr, Cdr, wT, a2, slab, slab_off):
        """Denoise_1/2 conv3 backward in one pass (zt_thin1x1_bwd_bf16): dr [1,H,W,8] bf16 gradient of the 1x1 output, wT the
        transposed-weight tensor of the data gradient ([1][48][8] bf16), a2 [1,H,W,>=48] bf16.  -> (dz2 [1,H,W,48] bf16, slabs written)."""
        import ctypes
        dr, a2 = _cv(dr), _cv(a2)
        assert dr.t.dtype == a2.t.dtype == wT.dtype == torch.bfloat16 and dr.ld == 8 and dr.N == 1 and (dr.H, dr.W) == (a2.H, a2.W)
        assert tuple(wT.shape[-2:]) == (48, 8) and a2.C >= 48
        dz = torch.empty((1, a2.H, a2.W, 48), dtype=torch.bfloat16, device=a2.t.device)
        n = ctypes.c_int(0)
        self.lib.call("zt_thin1x1_bwd_bf16", dr.ptr, Cdr, wT, a2.ptr, a2.ld, dz, 48, a2.H * a2.W, slab.data_ptr() + 4 * slab_off,
                      (slab.numel() - slab_off) * 4, ctypes.byref(n), self._s(a2.t))
        return dz, n.value

    @staticmethod
    def wgrad_slab_floats(Cin, Cout, K):
        c16 = lambda c: (c + 15) // 16 * 16
        return K * K * c16(Cin) * c16(Cout) + c16(Cout)

    def wgrad_reduce_multi(self, segs, accumulate=True):
        """segs: [(slab tensor, nslab, Cin, Cout, K, grad_w, grad_b)] -- one launch reduces every layer."""
        import ctypes
        n = len(segs)
        P, I = ctypes.c_void_p * n, ctypes.c_int * n
        dev = segs[0][0].device
        self.lib.call("zt_wgrad_reduce_multi_f32", n, P(*[s[0].data_ptr() for s in segs]), I(*[s[1] for s in segs]), I(*[s[2] for s in segs]),
                      I(*[s[3] for s in segs]), I(*[s[4] for s in segs]), P(*[s[5].data_ptr() for s in segs]),
                      P(*[(s[6].data_ptr() if s[6] is not None else None) for s in segs]), int(accumulate), current_stream(dev))

    def repack_weights_bf16_multi(self, entries):
        """entries: [(w fp32 [Cout,Cin,K,K], out bf16 [K*K,CoutP,ldk], transpose_flip)] -- all repacks of a step in one launch."""
        import ctypes
        n = len(entries)
        P, I = ctypes.c_void_p * n, ctypes.c_int * n
        dev = entries[0][0].device
        self.lib.call("zt_repack_conv_weights_bf16_multi", n, P(*[e[0].data_ptr() for e in entries]), P(*[e[1].data_ptr() for e in entries]),
                      I(*[e[0].shape[0] for e in entries]), I(*[e[0].shape[1] for e in entries]), I(*[e[0].shape[2] for e in entries]),
                      I(*[e[1].shape[1] for e in entries]), I(*[e[1].shape[2] for e in entries]), I(*[int(e[2]) for e in entries]),
                      current_stream(dev))

    def conv3x3_dgrad_bn_sums_bf16(self, dz, wT, res, zprev, scale, shift, mean):
        """Enhancer block backward: df = conv3x3^T(dz) + res and the BatchNorm-backward partial sums of the block below (whose
        pre-activation is zprev, BatchNorm constants scale / shift / mean) in one pass.  -> (df bf16 [1,H,W,64], part [512,2,64])."""
        dz, res, zp = _cv(dz), _cv(res), _cv(zprev)
        assert dz.t.dtype == res.t.dtype == zp.t.dtype == wT.dtype == torch.bfloat16 and dz.N == 1 and dz.C == 64 and zp.C == 64 and res.C == 64
        dev = dz.t.device
        df = torch.empty((1, dz.H, dz.W, 64), dtype=torch.bfloat16, device=dev)
        part = torch.empty((512, 2, 64), dtype=torch.float32, device=dev)
        tok = self._ev_begin(self.profile["match"].get((3, 3, 1, 64, 64, dz.H, dz.W))) if self.profile else None
        self.lib.call("zt_conv3x3_dgrad_bn_sums_bf16", dz.ptr, dz.ld, dz.H, dz.W, wT, wT.shape[1], wT.shape[2], df, 64, res.ptr, res.ld,
                      zp.ptr, zp.ld, scale, shift, mean, part, 512, self._s(dz.t))
        self._ev_end(tok)
        return df, part

    def conv3x3_bn_stats_bf16(self, x, wdev, bias, Cout):
        """y = conv3x3(x) + bias (bf16 nhwc) together with the BatchNorm statistics of y: -> (y, partial [1, 512, 2, Cout])."""
        x = _cv(x)
        assert x.t.dtype == torch.bfloat16 and wdev.dtype == torch.bfloat16 and x.N == 1 and wdev.shape[0] == 9
        out = torch.empty((1, x.H, x.W, Cout), dtype=torch.bfloat16, device=x.t.device)
        part = torch.empty((1, 512, 2, Cout), dtype=torch.float32, device=x.t.device)
        tok = self._ev_begin(self.profile["match"].get((3, 3, 1, x.C, Cout, x.H, x.W))) if self.profile else None
        self.lib.call("zt_conv3x3_bn_stats_bf16", x.ptr, x.ld, x.H, x.W, x.C, wdev, wdev.shape[1], wdev.shape[2], bias, out, Cout, Cout, part, 512,
                      self._s(x.t))
        self._ev_end(tok)
        return out, part

    def conv2d_wgrad_bf16(self, x, dz, Cout, KH, KW, grad_w, accumulate=False, slab=None, grad_b=None, relu_mask=None):
        """relu_mask: activation tensor (nhwc bf16) of the ReLU that follows the layer; dz is used as dz * [relu_mask > 0]."""
        x, dz = _cv(x), _cv(dz)
        mk = _cv(relu_mask) if relu_mask is not None else None
        assert x.t.dtype == torch.bfloat16 and dz.t.dtype == torch.bfloat16
        assert x.N == 1 and (x.H, x.W) == (dz.H, dz.W) and dz.C >= Cout
        assert tuple(grad_w.shape) == (Cout, x.C, KH, KW) and grad_w.is_contiguous() and grad_w.dtype == torch.float32
        slab = self.slab(x.t.device) if slab is None else slab
        self.lib.call("zt_conv2d_wgrad_nhwc_bf16", x.ptr, x.ld, dz.ptr, dz.ld, x.H, x.W, x.C, Cout, KH, KW, slab, slab.numel() * 4,
                      grad_w, grad_b, int(accumulate), mk.ptr if mk else None, mk.ld if mk else 0, self._s(x.t))
        return grad_w
