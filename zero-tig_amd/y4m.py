"""Raw video in and out (`predict.py --y4m_in / --y4m_out`): the YUV4MPEG2 container on the host, and the integer coefficients
the kernels of csrc/zt_yuv.hip consume.

A Y4M stream is one text line (`YUV4MPEG2 W.. H.. F..:.. I. A..:.. C... X...`) followed, per frame, by a `FRAME` line and the
payload: plane Y [H][W], then U, then V, 8 bits each (or 16 bits little-endian with the value in the low 9, 10, 12, 14 or 16 bits:
tags C420p10 ... C444p16).  Video tools read and write it through pipes
(`ffmpeg -i in.mp4 -f yuv4mpegpipe - | predict.py --y4m_in - --y4m_out - | ffmpeg -i - out.mp4`), so no decoder lives here.

`parse_header` -> `Header`; `Header.format(matrix)` -> `YuvFormat`, which fixes the conversion (subsampling, chroma siting, matrix,
range, depth) and carries the coefficient tables: round(c * 2^14) of the values derived from (Kr, Kb) in double precision;
round(c * 2^20), int64, for the 16-bit levels of a deep format (the same kernels at their deep scale).
`Y4MReader` is an iterator over payloads: one thread reads the stream into a bounded ring of (pinned) buffers, so the loop's
`next()` is a queue pop.  `Y4MWriter` follows `pngwriter.PngWriter`: a ring of pinned buffers, an asynchronous copy on the step's
stream plus an event per frame, a bounded queue, ONE thread per stream (frames land in order), `close()` drains and re-raises.
No processes are started."""
import collections
import queue
import re
import sys
import threading
import time

import numpy as np
import torch

S = 14                                              # coefficient precision of the kernels
S16 = 20                                            # the same for the deep formats (depth > 8)
DEPTHS = (8, 9, 10, 12, 14, 16)
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
# C tag -> (subsampling, siting): 0 = chroma centred between its two luma columns, 1 = co-sited with the left one
CTAGS = {"420jpeg": (420, 0), "420mpeg2": (420, 1), "420paldv": (420, 1), "420": (420, 1), "422": (422, 1), "444": (444, 0)}
# the deep tags have no siting variants: left for 420 / 422, as the bare C420
DEEP_CTAGS = {"%dp%d" % (ss, d): (ss, 0 if ss == 444 else 1, d) for ss in (420, 422, 444) for d in DEPTHS[1:]}


def ctag_info(ctag):
    """C tag -> (subsampling, siting, depth)"""
    return DEEP_CTAGS[ctag] if ctag in DEEP_CTAGS else CTAGS[ctag] + (8,)


def ctag_at_depth(ctag, depth):
    """the tag of the same subsampling at another depth: a deep tag carries no siting, so an 8-bit 420 tag maps to 420pN, and
    420pN maps back to 420mpeg2 (left siting, what the deep tag meant); at an unchanged depth the tag itself"""
    ss, _, d = ctag_info(ctag)
    if depth == d:
        return ctag
    return "%dp%d" % (ss, depth) if depth > 8 else {420: "420mpeg2", 422: "422", 444: "444"}[ss]


class YuvFormat(collections.namedtuple("YuvFormat", "W H ss siting matrix full depth", defaults=(8,))):
    """One planar Y'CbCr frame layout and its conversion: ss in (420, 422, 444), siting 0 centre / 1 left, matrix "bt601" /
    "bt709", full 0 (Y 16-235, chroma 16-240, times 2^(depth - 8)) / 1, depth 8 (one byte per sample) or 9, 10, 12, 14, 16 (uint16
    little-endian, the value in the low `depth` bits)."""
    __slots__ = ()

    def check(self):
        if self.depth not in DEPTHS:
            raise ValueError("yuv format: depth %r is not one of %s" % (self.depth, ", ".join(str(d) for d in DEPTHS)))
        if self.ss not in (420, 422, 444) or self.siting not in (0, 1) or (self.ss == 444 and self.siting != 0):
            raise ValueError("yuv format: subsampling %r with siting %r is not supported" % (self.ss, self.siting))
        if self.matrix not in KR_KB:
            raise ValueError("yuv format: matrix %r is not one of %s" % (self.matrix, sorted(KR_KB)))
        if self.W <= 0 or self.H <= 0 or (self.ss != 444 and self.W % 2) or (self.ss == 420 and self.H % 2):
            raise ValueError("yuv format: %dx%d does not divide into %d chroma samples" % (self.W, self.H, self.ss))
        return self

    @property
    def chroma_shape(self):
        return (self.H // 2 if self.ss == 420 else self.H, self.W if self.ss == 444 else self.W // 2)

    @property
    def frame_bytes(self):
        hc, wc = self.chroma_shape
        return (self.H * self.W + 2 * hc * wc) * (2 if self.depth > 8 else 1)

    def resized(self, W, H):
        return self._replace(W=int(W), H=int(H))

    def planes(self, payload):
        """numpy views (Y, U, V) of a payload (any 1-D uint8 array-like); uint16 views for depth > 8"""
        p = np.asarray(payload).reshape(-1)
        assert p.dtype == np.uint8 and p.size == self.frame_bytes, (p.dtype, p.size, self.frame_bytes)
        if self.depth > 8:
            p = p.view("<u2")
        hc, wc = self.chroma_shape
        n = self.H * self.W
        return p[:n].reshape(self.H, self.W), p[n:n + hc * wc].reshape(hc, wc), p[n + hc * wc:].reshape(hc, wc)

    def decode_coef(self):
        """int32 [6] on the host: yo, CY, CRV, CGU, CGV, CBU (zt_yuv_to_rgb_u8 / zt_yuv_to_planar_f32); for depth > 8 the int64
        table of zt_yuv16_to_planar_f32"""
        return _coef(self.matrix, self.full, self.depth)[0]

    def encode_coef(self):
        """int32 [10] on the host: yo, CYR, CYG, CYB, CUR, CUG, CUB, CVR, CVG, CVB (zt_rgb_f32_to_yuv); for depth > 8 the int64
        table of zt_rgb_f32_to_yuv16"""
        return _coef(self.matrix, self.full, self.depth)[1]


_COEF = {}


def _coef(matrix, full, depth):
    """(decode, encode) tables: RGB levels 0..255 against 8-bit samples, round(c * 2^14), int32; 0..65535 against samples
    of `depth` > 8 bits, round(c * 2^20), int64"""
    key = (matrix, int(bool(full)), int(depth))
    if key not in _COEF:
        kr, kb = KR_KB[matrix]
        kg = 1.0 - kr - kb
        levels, s, dtype = (255.0, S, torch.int32) if depth == 8 else (65535.0, S16, torch.int64)
        k = 1 << (depth - 8)
        yo, yr, cr = (0, (1 << depth) - 1, (1 << depth) - 1) if full else (16 * k, 219 * k, 224 * k)

        def q(v):
            return int(round(v * (1 << s)))
        cy, cs = levels / yr, levels / cr
        dec = [yo, q(cy), q(cs * 2 * (1 - kr)), q(cs * 2 * kb * (1 - kb) / kg), q(cs * 2 * kr * (1 - kr) / kg), q(cs * 2 * (1 - kb))]
        cyr, cyb = q(kr * yr / levels), q(kb * yr / levels)
        cur, cub = q(-kr / (2 * (1 - kb)) * cr / levels), q(0.5 * cr / levels)
        cvr, cvb = q(0.5 * cr / levels), q(-kb / (2 * (1 - kr)) * cr / levels)
        enc = [yo, cyr, q(yr / levels) - cyr - cyb, cyb, cur, -(cur + cub), cub, cvr, -(cvr + cvb), cvb]
        _COEF[key] = (torch.tensor(dec, dtype=dtype), torch.tensor(enc, dtype=dtype))
    return _COEF[key]


def encode_host(rgb, fmt):
    """uint8 [H][W][3] -> payload (numpy): the encode of zt_rgb_f32_to_yuv on the host, in int64, from the same coefficient table.
    A deep format (depth > 8) takes uint16 [H][W][3], 16-bit levels, and gives the encode of zt_rgb_f32_to_yuv16.
    For tools that have to make a stream without a device; tests/test_y4m.py and test_y4m_deep.py restate the definitions on their own."""
    yo, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb = (int(v) for v in fmt.check().encode_coef())
    deep = fmt.depth > 8
    assert np.asarray(rgb).dtype == (np.uint16 if deep else np.uint8), (np.asarray(rgb).dtype, fmt.depth)
    S, mid, top, dtype = (S16, 1 << (fmt.depth - 1), (1 << fmt.depth) - 1, "<u2") if deep else (14, 128, 255, np.uint8)
    R, G, B = (np.asarray(rgb)[..., i].astype(np.int64) for i in range(3))
    Y = yo + ((cyr * R + cyg * G + cyb * B + (1 << (S - 1))) >> S)

    def foot(P):
        if fmt.ss == 444:
            return P
        if fmt.siting == 0:
            s = P[:, 0::2] + P[:, 1::2]
        else:
            s = P[:, np.maximum(np.arange(0, fmt.W, 2) - 1, 0)] + 2 * P[:, 0::2] + P[:, 1::2]
        return s[0::2] + s[1::2] if fmt.ss == 420 else s
    sh = (0 if fmt.ss == 444 else 1 if fmt.siting == 0 else 2) + (1 if fmt.ss == 420 else 0)
    Rs, Gs, Bs = foot(R), foot(G), foot(B)
    U = mid + ((cur * Rs + cug * Gs + cub * Bs + (1 << (S - 1 + sh))) >> (S + sh))
    V = mid + ((cvr * Rs + cvg * Gs + cvb * Bs + (1 << (S - 1 + sh))) >> (S + sh))
    return np.concatenate([np.clip(p, 0, top).astype(dtype).reshape(-1) for p in (Y, U, V)]).view(np.uint8)


# ---- the container ----------------------------------------------------------------------------------------------------------------
MAGIC = b"YUV4MPEG2"


class Header(collections.namedtuple("Header", "W H fps interlace aspect ctag color_range")):
    """fps / aspect: "num:den" strings or None; interlace: "p", "?" or None; ctag: a key of CTAGS or DEEP_CTAGS ("420" when the
    stream has no C parameter); color_range: the XCOLORRANGE value ("FULL", "LIMITED") or None."""
    __slots__ = ()

    @property
    def full(self):
        return int(self.color_range == "FULL")

    def format(self, matrix="bt709"):
        ss, siting, depth = ctag_info(self.ctag)
        return YuvFormat(self.W, self.H, ss, siting, matrix, self.full, depth).check()

    def resized(self, W, H):
        return self._replace(W=int(W), H=int(H))

    def to_bytes(self):
        parts = [MAGIC.decode(), "W%d" % self.W, "H%d" % self.H]
        if self.fps:
            parts.append("F" + self.fps)
        if self.interlace:
            parts.append("I" + self.interlace)
        if self.aspect:
            parts.append("A" + self.aspect)
        parts.append("C" + self.ctag)
        if self.color_range:
            parts.append("XCOLORRANGE=" + self.color_range)
        return (" ".join(parts) + "\n").encode("ascii")


def parse_header(line, max_depth=8):
    """The stream's first line (bytes, with or without the newline) -> Header.  Raises ValueError naming the field it rejects.
    `max_depth`: the deepest sample a caller takes; 8 rejects the deep tags (C420p10 ...), 16 accepts every one of DEEP_CTAGS."""
    try:
        text = bytes(line).decode("ascii").rstrip("\n")
    except UnicodeDecodeError:
        raise ValueError("y4m: the header is not ASCII text") from None
    tok = text.split(" ")
    if tok[0] != MAGIC.decode():
        raise ValueError("y4m: the stream does not start with %s" % MAGIC.decode())
    f = {"W": None, "H": None, "F": None, "I": None, "A": None, "C": None}
    color_range = None
    for t in [t for t in tok[1:] if t]:
        if t[0] == "X":
            if t.startswith("XCOLORRANGE="):
                color_range = t.split("=", 1)[1].upper()
        elif t[0] in f:
            f[t[0]] = t[1:]
        else:
            raise ValueError("y4m: unknown header field %r" % t)
    try:
        W, H = int(f["W"]), int(f["H"])
        assert W > 0 and H > 0
    except (TypeError, ValueError, AssertionError):
        raise ValueError("y4m: fields W / H: width and height must be positive integers, got W%s H%s" % (f["W"], f["H"])) from None
    if f["I"] not in (None, "p", "?"):
        raise ValueError("y4m: field I%s: interlaced streams are not supported (Ip or I? only)" % f["I"])
    ctag = "420" if f["C"] is None else f["C"]
    if ctag not in CTAGS and not (ctag in DEEP_CTAGS and DEEP_CTAGS[ctag][2] <= max_depth):
        why = ("more than 8 bits per sample" if re.search(r"p\d+$", ctag) or ctag == "mono16" else
               "no chroma planes" if ctag.startswith("mono") else "an alpha plane" if "alpha" in ctag else "unknown layout")
        deep = [c for c, v in DEEP_CTAGS.items() if v[2] <= max_depth]
        raise ValueError("y4m: field C%s is not supported (%s); one of %s" % (ctag, why, ", ".join("C" + c for c in list(CTAGS) + deep)))
    if color_range not in (None, "FULL", "LIMITED"):
        raise ValueError("y4m: field XCOLORRANGE=%s: FULL or LIMITED" % color_range)
    ss = ctag_info(ctag)[0]
    if (ss != 444 and W % 2) or (ss == 420 and H % 2):
        raise ValueError("y4m: fields W%d H%d: odd sizes cannot carry C%s chroma" % (W, H, ctag))
    for k in ("F", "A"):
        if f[k] is not None:
            nd = f[k].split(":")
            if len(nd) != 2 or not all(v.isdigit() for v in nd):
                raise ValueError("y4m: field %s%s is not num:den" % (k, f[k]))
    return Header(W, H, f["F"], f["I"], f["A"], ctag, color_range)


def _alloc(nbytes, pin):
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=bool(pin))


def _open_in(path):
    return (sys.stdin.buffer, False) if path == "-" else (open(path, "rb"), True)


def _seekable(fh):
    try:
        return bool(fh.seekable())
    except (AttributeError, ValueError):
        return False


def count_frames(path):
    """the number of frames of a Y4M file: the header is parsed, then per frame the FRAME line is read and the payload stepped over
    with a seek (no payload is read, nothing touches the GPU).  A last frame with fewer bytes than the header promises raises the
    reader's ValueError; a pipe cannot be counted."""
    with open(path, "rb") as fh:
        if not _seekable(fh):
            raise ValueError("y4m: %s is not seekable: its frames cannot be counted" % path)
        line = fh.readline(1024)
        if not line.endswith(b"\n"):
            raise ValueError("y4m: no header line in the first %d bytes" % len(line))
        frame_bytes = parse_header(line, max_depth=16).format().frame_bytes
        size = fh.seek(0, 2)
        fh.seek(len(line))
        n = 0
        while True:
            line = fh.readline(1024)
            if not line:
                return n
            if not (line.startswith(b"FRAME") and line.endswith(b"\n")):
                raise ValueError("y4m: frame %d: expected a FRAME line, got %r" % (n, line[:32]))
            pos = fh.tell()
            if pos + frame_bytes > size:
                raise ValueError("y4m: truncated stream: frame %d has %d of %d bytes" % (n, size - pos, frame_bytes))
            fh.seek(frame_bytes, 1)
            n += 1


def rank_share(n, rank, world):
    """frames of an n-frame stream that `rank` of `world` trains on -> (first, count, steps_per_epoch): contiguous shares of
    per = ceil(n / world) frames, as train.py cuts the frame list of a dataset (the last shares may be short or empty);
    every rank takes `steps_per_epoch` = the smallest share, so that all of them make the same number of all-reduces."""
    assert n >= 0 and world >= 1 and 0 <= rank < world, (n, rank, world)
    per = (n + world - 1) // world
    shares = [max(min(n, (r + 1) * per) - r * per, 0) for r in range(world)]
    return rank * per, shares[rank], min(shares)


class Y4MReader:
    """reader = Y4MReader(path or "-"); reader.header; for payload in reader: ...

    `payload` is a 1-D uint8 tensor of `header.format().frame_bytes` bytes in a ring buffer (pinned when a GPU is there, `pin=`
    overrides).  It is valid until the next `next()`; `release(event)` hands it back earlier and makes the reader thread wait for
    `event` (the asynchronous copy to the device) before it overwrites the buffer -- a loop that copies with non_blocking=True
    must release with that event.  A stream that ends inside a frame raises ValueError; a clean end of file ends the iteration.
    `wait` accumulates the seconds `next()` spent blocked.

    `first` / `count`: the iteration covers frames first .. first + count - 1 of the stream (count None = to the end; a share of
    `train.py`'s ranks).  On a seekable file the frames before `first` are stepped over (the FRAME line is read, the payload
    skipped with a seek); on a pipe they are read and dropped.  A `first` past the end gives an empty iteration."""

    def __init__(self, path, slots=4, pin=None, fh=None, first=0, count=None):
        assert slots >= 2 and first >= 0 and (count is None or count >= 0), (slots, first, count)
        self._first, self._count = int(first), None if count is None else int(count)
        self._fh, self._own = (fh, False) if fh is not None else _open_in(path)
        line = self._fh.readline(1024)
        if not line.endswith(b"\n"):
            raise ValueError("y4m: no header line in the first %d bytes" % len(line))
        self.header = parse_header(line, max_depth=16)
        self.frame_bytes = self.header.format().frame_bytes
        pin = torch.cuda.is_available() if pin is None else pin
        self._free, self._full = queue.Queue(), queue.Queue(maxsize=slots)
        for _ in range(slots):
            self._free.put((_alloc(self.frame_bytes, pin), None))
        self._held, self._stop, self.wait, self.frames = None, False, 0.0, 0
        self._thread = threading.Thread(target=self._run, name="y4m-reader", daemon=True)
        self._thread.start()

    def _skip(self):
        """step over the frames before `first` -> False when the stream ends there"""
        seekable = _seekable(self._fh)
        for n in range(self._first):
            line = self._fh.readline(1024)
            if not line:
                return False
            if not (line.startswith(b"FRAME") and line.endswith(b"\n")):
                raise ValueError("y4m: frame %d: expected a FRAME line, got %r" % (n, line[:32]))
            if seekable:
                self._fh.seek(self.frame_bytes, 1)
            else:
                left = self.frame_bytes
                while left:
                    k = len(self._fh.read(min(left, 1 << 20)))
                    if not k:
                        raise ValueError("y4m: truncated stream: frame %d has %d of %d bytes" % (n, self.frame_bytes - left, self.frame_bytes))
                    left -= k
        return True

    def _run(self):
        n = self._first
        try:
            more = self._skip()
            while more and (self._count is None or n < self._first + self._count):
                item = self._free.get()
                if item is None:
                    return
                buf, event = item
                if event is not None:
                    event.synchronize()
                line = self._fh.readline(1024)
                if not line:                                # clean end of stream
                    break
                if not (line.startswith(b"FRAME") and line.endswith(b"\n")):
                    raise ValueError("y4m: frame %d: expected a FRAME line, got %r" % (n, line[:32]))
                view, got = memoryview(buf.numpy()), 0
                while got < self.frame_bytes:
                    k = self._fh.readinto(view[got:])
                    if not k:
                        raise ValueError("y4m: truncated stream: frame %d has %d of %d bytes" % (n, got, self.frame_bytes))
                    got += k
                self._full.put(buf)
                n += 1
            self._full.put(None)
        except BaseException as e:                          # noqa: BLE001 -- raised by next()
            self._full.put(e)

    def release(self, event=None):
        """hand the frame of the last `next()` back to the ring; `event`: work that still reads it"""
        if self._held is not None:
            self._free.put((self._held, event))
            self._held = None

    def __iter__(self):
        return self

    def __next__(self):
        self.release()
        if self._stop:
            raise StopIteration
        t0 = time.perf_counter()
        item = self._full.get()
        self.wait += time.perf_counter() - t0
        if item is None or isinstance(item, BaseException):
            self._stop = True
            self.close()
            if item is None:
                raise StopIteration
            raise item
        self._held = item
        self.frames += 1
        return item

    def close(self, timeout=2.0):
        """stop the reader thread and wait for it.  At the end of the stream the thread has already returned; closed earlier it
        stops at its next buffer request (the queue is drained so that it is not blocked there).  A thread inside read() on a
        pipe that nobody feeds cannot be interrupted: after `timeout` seconds it is left behind as a daemon, with the file open."""
        self._stop = True
        self._free.put(None)
        deadline = time.perf_counter() + timeout
        while self._thread.is_alive() and time.perf_counter() < deadline:
            try:
                self._full.get_nowait()
            except queue.Empty:
                pass
            self._thread.join(0.02)
        if self._own and not self._thread.is_alive():
            self._fh.close()
            self._own = False


class Y4MWriter:
    """writer = Y4MWriter(path or "-", header); writer.submit(payload) per frame; writer.close() at the end.

    `submit` takes the device payload `InferStep.yuv` holds (an asynchronous copy into a pinned ring buffer is enqueued on the
    current stream, followed by an event: work enqueued afterwards may overwrite the payload) or host bytes.  One thread writes the
    header, then `FRAME\\n` + payload per frame, in submission order.  The ring and the queue are bounded (`slots`), so a slow sink
    blocks `submit` (`wait_writer`; `thread_event` / `thread_io` tell a slow device from a slow sink); an exception of the thread (a closed pipe, a full disk) is re-raised by the next `submit` and by `close()`.
    `open_fn(path, "wb")` opens the output (tests substitute it); "-" is the process's standard output, `fh=` any binary file."""

    def __init__(self, path, header, slots=4, open_fn=open, fh=None):
        assert slots >= 1
        self.header, self.frame_bytes = header, header.format().frame_bytes
        self._path, self._open, self._fh, self._own = path, open_fn, fh, False
        self._jobs, self._free = queue.Queue(maxsize=slots), queue.Queue()
        for _ in range(slots):
            self._free.put(None)                            # buffers are allocated on first use
        self._error, self._closed = None, False
        self.wait_writer, self.frames, self.bytes = 0.0, 0, 0
        self.thread_event, self.thread_io = 0.0, 0.0      # seconds the thread waited for the device / spent in write()
        self._thread = threading.Thread(target=self._run, name="y4m-writer", daemon=True)
        self._thread.start()

    def _check(self):
        if self._error is not None:
            raise self._error
        assert not self._closed, "Y4MWriter is closed"

    def submit(self, payload):
        self._check()
        t0 = time.perf_counter()
        if isinstance(payload, torch.Tensor) and payload.device.type == "cuda":
            assert payload.dtype == torch.uint8 and payload.numel() == self.frame_bytes, (payload.dtype, payload.numel())
            buf = self._free.get()
            self.wait_writer += time.perf_counter() - t0
            if buf is None:
                buf = _alloc(self.frame_bytes, True)
            buf.copy_(payload.view(-1), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            job = (buf.numpy(), done, buf)
        else:
            data = memoryview(payload.numpy() if isinstance(payload, torch.Tensor) else payload).cast("B")
            assert len(data) == self.frame_bytes, (len(data), self.frame_bytes)
            job = (data, None, None)
        t0 = time.perf_counter()
        self._jobs.put(job)
        self.wait_writer += time.perf_counter() - t0

    def close(self):
        """drain the queue, stop the thread, flush; re-raise the first exception the thread met"""
        if not self._closed:
            self._closed = True
            self._jobs.put(None)
            self._thread.join()
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                               # do not mask the loop's own exception
            try:
                self.close()
            except Exception:
                pass
        return False

    def _start(self):
        if self._fh is None:
            if self._path == "-":
                self._fh = sys.stdout.buffer
            else:
                self._fh, self._own = self._open(self._path, "wb"), True
        self._fh.write(self.header.to_bytes())

    def _run(self):
        started = False
        while True:
            job = self._jobs.get()
            try:
                if self._error is None:                     # after a failure the remaining jobs are only released
                    if not started:
                        started = True
                        self._start()
                    if job is not None:
                        data, done, _ = job
                        t0 = time.perf_counter()
                        if done is not None:
                            done.synchronize()
                        t1 = time.perf_counter()
                        self._fh.write(b"FRAME\n")
                        self._fh.write(data)
                        self.thread_event += t1 - t0
                        self.thread_io += time.perf_counter() - t1
                        self.frames += 1
                        self.bytes += 6 + len(data)
                    else:
                        self._fh.flush()
                        if self._own:
                            self._fh.close()
            except BaseException as e:                      # noqa: BLE001 -- surfaced by close() / the next submit
                if self._error is None:
                    self._error = e
            finally:
                if job is not None and job[2] is not None:
                    self._free.put(job[2])
            if job is None:
                return


def write_file(path, header, payloads):
    """a complete stream from host payloads (tests, tools)"""
    with open(path, "wb") as fh:
        fh.write(header.to_bytes())
        for p in payloads:
            fh.write(b"FRAME\n")
            fh.write(memoryview(np.ascontiguousarray(p)).cast("B"))
