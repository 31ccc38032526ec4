"""Streaming inference: `InferStep`, the inference twin of `optim.TrainStep`.

`Finetunemodel.forward` launches every kernel eagerly and repacks the nine weight tensors per frame; that form stays as the
parity-pinned API of the reference.  `InferStep` runs the same model for frozen weights: the weights are prepared once per
binding (device layouts, eval-mode BatchNorm folded into enhance.conv.0), the frame is enhanced by `Engine.forward_stream`, the
two uint8 images the scripts write are made inside the step, and the steady-state frame is one hipGraph replay."""
import torch


class InferStep:
    """One frame of the inference loop (reference predict.py:40-55) as a callable:

        step = InferStep(model, use_graph=True, ingest_size=(1920, 1080))
        H2, H3, s3 = step(frame, is_new_seq)      # the three tensors of Finetunemodel.forward
        enh_u8, out_u8 = step.u8                  # uint8 [H,W,3] device tensors of H2 / H3 (truncating quantisation, predict.py:57-61)
        enh_png, out_png = step.png               # png=True: (zlib stream, byte count) of each, as `Ops.png_encode` returns them

    `frame` is fp32 [1,3,H,W], or a decoded uint8 frame ([H0,W0,3] / [1,H0,W0,3]) which goes through the ingest kernels
    (`ingest_size` = (W, H) it is resized to, None = keep).  The recurrent cache update (`model.update_H3`) is part of the step.

    png=True: both uint8 images are also deflated inside the step (and inside the captured graph) into the zlib streams of their
    PNG files (predict.py:101-104); `pngwriter.PngWriter.submit` copies and writes them.  png=2: the same with the encoder's
    mode 2 (run-length matches where a block has runs, `Ops.png_encode(.., mode=2)`); True means mode 1.

    use_graph=False: eager launches of the streaming plan.  use_graph=True: the frame is copied into a static input buffer and
    the recurrent cache lives in static buffers; new-sequence frames and the first steady-state frame run eagerly, the second
    steady-state frame is captured into a hipGraph (RAFT's side stream becomes a parallel branch, as in `TrainStep`) and later
    frames replay it.  A change of the frame shape captures again.

    THE RETURNED TENSORS, `step.u8` AND `step.png` LIVE IN THE STEP'S (GRAPH'S) BUFFERS: they are valid until the next call; copy what must
    survive it.  The model must not be moved, and `last_H3 / last_s3` not re-assigned by the caller, after the capture.

    yuv=fmt (a `y4m.YuvFormat`: W, H, subsampling, chroma siting, matrix, range): `frame` is the 1-D uint8 payload of a raw video
    frame (planes Y, U, V), pinned or on the device.  It is copied into a static device buffer (`step.loaded` is the event behind
    that copy: the host buffer may be reused once it has completed) and converted inside the step -- `Ops.yuv_to_planar_f32`
    straight into the input when `ingest_size` is None or (W, H), `Ops.yuv_to_rgb_u8` + `Ops.ingest_u8` otherwise -- and
    `step.yuv = (enhance_payload, denoise_payload)` holds the two results as payloads of the SAME subsampling, siting, matrix and
    range at the output size (`step.yuv_format`), made from H2 / H3 by `Ops.rgb_f32_to_yuv`.  All of it is part of the captured
    graph; `step.u8` / `step.png` are filled as without it.  `yuv_out_depth` (None = the input's) sets the depth of the two output
    payloads alone: an 8-bit stream can leave as 10-bit and the other way round; which conversion runs is decided here, at
    construction, so the captured graph has no branch.  A deep input (depth > 8) is never resized: `ingest_size` other than None
    or (W, H) raises ValueError.

    yuv_size=(W, H) (needs yuv= and ingest_size=None): the payload is decoded at the stream's size and resized in float by
    `Ops.yuv_to_planar_f32_sized` (Pillow's mode-F BICUBIC) inside the step, so also inside the captured graph; it works at
    every depth, its buffers are allocated once, and `step.yuv_format` is `fmt.resized(W, H)` at the output depth.

    Weights are prepared again when a parameter or BatchNorm buffer changed (`_version` / `data_ptr()` of the tensors, e.g. after
    `load_state_dict`); the prepared buffers keep their addresses, so a captured graph stays valid across a reload."""

    def __init__(self, model, use_graph=True, ingest_size=(1920, 1080), png=False, yuv=None, yuv_out_depth=None, yuv_size=None):
        assert int(png) in (0, 1, 2), png
        self.model, self.use_graph, self.ingest_size, self.want_png = model, use_graph, ingest_size, int(png)
        self.graph, self.x, self.out, self.u8, self.png = None, None, None, None, None
        self.fmt, self.yuv, self.yuv_format, self.loaded, self._payload = yuv, None, None, None, None
        assert yuv is not None or yuv_out_depth is None, "yuv_out_depth needs yuv="
        self.yuv_size, self._sized = None, None
        if yuv_size is not None:
            if yuv is None or ingest_size is not None:
                raise ValueError("InferStep: yuv_size needs yuv= and ingest_size=None (got yuv=%r, ingest_size=%r)" % (yuv, ingest_size))
            self.yuv_size = (int(yuv_size[0]), int(yuv_size[1]))
        if yuv is not None:
            yuv.check()
            W, H = self.yuv_size if self.yuv_size is not None else (yuv.W, yuv.H) if ingest_size is None else ingest_size
            if yuv.depth > 8 and (W, H) != (yuv.W, yuv.H) and self.yuv_size is None:
                raise ValueError("InferStep: a %d-bit input cannot be resized (%dx%d -> %dx%d): the resize is 8-bit; use ingest_size=None, and yuv_size=(W, H) for the float resize"
                                 % (yuv.depth, yuv.W, yuv.H, W, H))
            # the output streams: same layout at the output size, at the input's depth unless another is asked for
            self.yuv_format = yuv.resized(W, H)._replace(depth=yuv.depth if yuv_out_depth is None else int(yuv_out_depth)).check()
        self.n_eager_steady, self.n_captures, self.n_prepares = 0, 0, 0
        self._wp, self._wsig, self._bound = None, None, None

    # ---- frozen weights -----------------------------------------------------------------------------------------------------
    def _tensors(self):
        m = self.model
        bn = m.enhance.conv[1]
        return [p for _, p in m._trainable()] + [bn.running_mean, bn.running_var]

    def _prepare(self):
        """-> (engine, RAFT plan) with the prepared weight table current"""
        eng, rp = self.model._plan()
        bound = (eng, eng.precision)              # the engine object itself: a replaced engine (model.to(), new precision) never compares equal
        if self._bound is None or self._bound[0] is not eng or self._bound[1] != eng.precision:
            # the model moved / changed precision: new buffers, and no graph holds the old ones
            self._bound, self._wp, self._wsig, self.graph, self.n_eager_steady = bound, None, None, None, 0
        sig = tuple((t.data_ptr(), t._version) for t in self._tensors())
        if sig != self._wsig:
            with torch.no_grad():
                self._wp = eng.prepare_stream(self._wp)
            self._wsig = sig
            self.n_prepares += 1
        return eng, rp

    # ---- one frame ----------------------------------------------------------------------------------------------------------
    def _load(self, frame, dev, out=None):
        """frame -> fp32 [1,3,H,W] on the device (uint8 frames through `Ops.ingest_u8`, as `TrainStep._load`)"""
        if frame.dtype == torch.uint8:
            self.model._plan()
            return self.model._ops.ingest_u8(frame.to(dev, non_blocking=True), out=out, size=self.ingest_size)
        if out is None:
            return frame.to(dev, non_blocking=True).detach().contiguous().float()
        out.copy_(frame, non_blocking=True)
        return out

    def _load_yuv(self, frame, dev):
        """payload -> the device buffer the conversion reads (static when the step is graph-replayed)"""
        assert frame.dtype == torch.uint8 and frame.dim() == 1 and frame.numel() == self.fmt.frame_bytes, \
            (frame.dtype, tuple(frame.shape), self.fmt.frame_bytes)
        if self._payload is None or self._payload.device != dev:
            self._payload = torch.empty(self.fmt.frame_bytes, dtype=torch.uint8, device=dev)
        self._payload.copy_(frame, non_blocking=True)
        self.loaded = torch.cuda.Event()
        self.loaded.record()
        return self._payload

    def _decode(self, ops, payload, x):
        """the payload in `self._payload` -> the model's input (x: the static input buffer, or None)"""
        if self.yuv_format[:2] == self.fmt[:2]:
            return ops.yuv_to_planar_f32(payload, self.fmt, out=x)
        if self.yuv_size is not None:
            if self._sized is None or self._sized["decode"].device != payload.device:
                self._sized = ops.sized_bufs(self.fmt, self.yuv_size, payload.device)
            return ops.yuv_to_planar_f32_sized(payload, self.fmt, self.yuv_size, out=x, bufs=self._sized)
        return ops.ingest_u8(ops.yuv_to_rgb_u8(payload, self.fmt), out=x, size=self.ingest_size)

    def _body(self, eng, rp, x, payload=None):
        m = self.model
        if payload is not None:
            x = self._decode(eng.ops, payload, x)
        new = m.is_new_seq or m.last_H3 is None
        cache_fn = None if new else (lambda L2: rp.update_cache(m.last_H3, m.last_s3, L2, m.of_scale))
        H2, H3, s3 = eng.forward_stream(x, cache_fn, self._wp)
        m.last_H3_wp, m.last_s3_wp = eng.last_wp
        m.update_H3(H3, s3)
        u8 = (eng.ops.quantize_u8(H2, 0), eng.ops.quantize_u8(H3, 0))
        png = tuple(eng.ops.png_encode(u, mode=self.want_png) for u in u8) if self.want_png else None
        yuv = None if payload is None else (eng.ops.rgb_f32_to_yuv(H2, self.yuv_format), eng.ops.rgb_f32_to_yuv(H3, self.yuv_format))
        return (H2, H3, s3), u8, png, yuv

    def __call__(self, frame, is_new_seq=False):
        m = self.model
        m.is_new_seq = bool(is_new_seq)
        dev = m._trainable()[0][1].device
        eng, rp = self._prepare()
        with torch.no_grad():
            payload = None if self.fmt is None else self._load_yuv(frame, dev)
            if not self.use_graph:
                self.out, self.u8, self.png, self.yuv = self._body(eng, rp, None if self.fmt else self._load(frame, dev), payload)
                return self.out
            if self.fmt is not None:
                shape = (1, 3, self.yuv_format.H, self.yuv_format.W)
            elif frame.dtype == torch.uint8:
                Wi, Hi = self.ingest_size if self.ingest_size is not None else (frame.shape[-2], frame.shape[-3])
                shape = (1, 3, Hi, Wi)
            else:
                shape = tuple(frame.shape)
            if self.x is not None and tuple(self.x.shape) != shape:      # the captured launch sequence no longer applies
                self.graph, self.n_eager_steady, self.x = None, 0, None
            if self.x is None:
                self.x = torch.empty(shape, dtype=torch.float32, device=dev)
                m.enable_static_cache(shape)
            if self.fmt is None:
                self._load(frame, dev, out=self.x)
            if is_new_seq or m.last_H3 is None or self.n_eager_steady < 1:
                # eager: new-sequence frames, and the first steady-state frame (loads every kernel's code object and sizes the
                # RAFT plan's buffers before anything is captured)
                if not (is_new_seq or m.last_H3 is None):
                    self.n_eager_steady += 1
                self.out, self.u8, self.png, self.yuv = self._body(eng, rp, self.x, payload)
                return self.out
            if self.graph is None:
                torch.cuda.synchronize(dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._gout = self._body(eng, rp, self.x, payload)
                self.graph = g
                self.n_captures += 1
            self.graph.replay()
            self.out, self.u8, self.png, self.yuv = self._gout
            return self.out
