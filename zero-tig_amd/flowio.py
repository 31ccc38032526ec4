"""Middlebury .flo files (`evals.py --tc_flo_dir`, `utils/frame_utils.py`): the float32 tag 202021.25, int32 width, int32 height,
then the rows of interleaved (u, v) float32, everything little-endian.

`write_flo` / `read_flo` work on host arrays [H, W, 2].  `FloWriter` follows `y4m.Y4MWriter`: a ring of pinned buffers, an
asynchronous copy on the current stream plus an event per flow, a bounded queue and ONE thread that writes one file per flow, in
submission order; the loop waits only when it runs out of slots, and an exception of the thread (a full disk, a missing
directory) is re-raised by the next `submit` and by `close()`.  No processes are started."""
import queue
import struct
import threading
import time

import numpy as np
import torch

TAG = 202021.25
_TAG_BYTES = struct.pack("<f", TAG)                 # b"PIEH"


def _head(w, h):
    return _TAG_BYTES + struct.pack("<ii", int(w), int(h))


def write_flo(path, flow):
    """flow: [H, W, 2], anything numpy converts to float32"""
    a = np.ascontiguousarray(np.asarray(flow), dtype="<f4")
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError("%s: a flow is [H, W, 2]; got %s" % (path, (a.shape,)))
    with open(path, "wb") as fh:
        fh.write(_head(a.shape[1], a.shape[0]))
        fh.write(memoryview(a).cast("B"))


def read_flo(path):
    """-> float32 [H, W, 2]; a wrong tag, a size that is not positive or a file that is shorter or longer than its header says
    raise ValueError naming the path"""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) < 12:
        raise ValueError("%s: not a .flo file: %d bytes, the header alone has 12" % (path, len(data)))
    if data[:4] != _TAG_BYTES:
        raise ValueError("%s: not a .flo file: the tag is %r, not %r (202021.25 as little-endian float32)" % (path, data[:4], _TAG_BYTES))
    w, h = struct.unpack("<ii", data[4:12])
    if w < 1 or h < 1:
        raise ValueError("%s: the header says %d x %d" % (path, w, h))
    if len(data) != 12 + 8 * w * h:
        raise ValueError("%s: %d x %d needs %d bytes, the file has %d" % (path, w, h, 12 + 8 * w * h, len(data)))
    return np.frombuffer(data, dtype="<f4", offset=12).reshape(h, w, 2).astype(np.float32)


class FloWriter:
    """writer = FloWriter(); writer.submit(path, flow) per flow; writer.close() at the end.

    `flow`: float32 [H, W, 2] (what `Ops.flow_pack` returns) on the device -- an asynchronous copy into a pinned buffer is enqueued
    on the current stream, followed by an event: work enqueued afterwards may overwrite the tensor -- or on the host (copied before
    `submit` returns).  `wait_writer`: seconds `submit` waited for a free slot; `thread_event` / `thread_io`: seconds the thread
    waited for the device / spent writing."""

    def __init__(self, slots=4, open_fn=open):
        assert slots >= 1
        self._open = open_fn
        self._jobs, self._free = queue.Queue(maxsize=slots), queue.Queue()
        for _ in range(slots):
            self._free.put(None)                            # buffers are allocated on first use
        self._error, self._closed = None, False
        self.wait_writer, self.files, self.bytes = 0.0, 0, 0
        self.thread_event, self.thread_io = 0.0, 0.0
        self._thread = threading.Thread(target=self._run, name="flo-writer", daemon=True)
        self._thread.start()

    def _check(self):
        if self._error is not None:
            raise self._error
        assert not self._closed, "FloWriter is closed"

    def submit(self, path, flow):
        self._check()
        if isinstance(flow, np.ndarray):
            flow = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32))
        assert flow.dtype == torch.float32 and flow.dim() == 3 and flow.shape[2] == 2 and flow.is_contiguous(), (flow.dtype, tuple(flow.shape))
        h, w = int(flow.shape[0]), int(flow.shape[1])
        t0 = time.perf_counter()
        if flow.device.type == "cuda":
            buf = self._free.get()
            if buf is None or buf.numel() != flow.numel():
                buf = torch.empty(flow.numel(), dtype=torch.float32, pin_memory=True)
            buf.copy_(flow.view(-1), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            job = (path, w, h, buf.numpy(), done, buf)
        else:
            job = (path, w, h, flow.detach().clone().view(-1).numpy(), None, None)
        self._jobs.put(job)
        self.wait_writer += time.perf_counter() - t0

    def close(self):
        """drain the queue, stop the thread; re-raise the first exception the thread met"""
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

    def _run(self):
        while True:
            job = self._jobs.get()
            try:
                if job is not None and self._error is None:  # after a failure the remaining jobs are only released
                    path, w, h, data, done, _ = job
                    t0 = time.perf_counter()
                    if done is not None:
                        done.synchronize()
                    t1 = time.perf_counter()
                    with self._open(path, "wb") as fh:
                        fh.write(_head(w, h))
                        fh.write(memoryview(data).cast("B"))
                    self.thread_event += t1 - t0
                    self.thread_io += time.perf_counter() - t1
                    self.files += 1
                    self.bytes += 12 + 8 * w * h
            except BaseException as e:                      # noqa: BLE001 -- surfaced by close() / the next submit
                if self._error is None:
                    self._error = e
            finally:
                if job is not None and job[5] is not None:
                    self._free.put(job[5])
            if job is None:
                return
