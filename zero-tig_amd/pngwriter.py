"""Host side of the device PNG path (`--device_png 1` of predict.py / evals.py): `Ops.png_encode` leaves a finished zlib stream in
device memory; this module frames it as a PNG file and writes it, off the inference loop's thread.

`PngWriter` owns a small ring of pinned host buffers.  `submit` copies each stream's byte count to the host, waits for it (that is
the wait for the step itself), and enqueues a copy of exactly that many bytes on the step's stream followed by an event: the next
step is ordered behind the copy and may overwrite the step's buffers, and a writer thread picks the job up once the event has
completed.  At most two threads frame the chunks (zlib.crc32 releases the GIL) and write; no processes are started.  Both the
ring and the job queue are bounded, so a slow disk blocks `submit` instead of growing memory.  `close()` drains the queue and
re-raises the first exception of a worker."""
import queue
import struct
import threading
import time
import zlib

import torch

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def png_frame(stream, height, width, idat_bytes=1 << 20):
    """zlib stream of an 8-bit RGB image's filtered scanlines (bytes-like) -> the complete PNG file as a list of byte strings:
    signature, IHDR (8-bit, colour type 2, no interlace), IDAT chunks of at most `idat_bytes`, IEND; CRCs by zlib.crc32."""
    def chunk(tag, data):
        return [struct.pack(">I", len(data)), tag, data, struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)))]
    view = memoryview(stream).cast("B")
    parts = [PNG_SIGNATURE] + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))
    for o in range(0, max(len(view), 1), idat_bytes):
        parts += chunk(b"IDAT", view[o:o + idat_bytes])
    return parts + chunk(b"IEND", b"")


class _Slot:
    def __init__(self):
        self.buf, self.count = None, None

    def reserve(self, nbytes):
        if self.count is None:
            self.count = torch.empty(1, dtype=torch.int32, pin_memory=True)
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)


class PngWriter:
    """writer = PngWriter(); writer.submit([(path, stream, nbytes, H, W), ...]) per frame; writer.close() at the end.

    slots: pinned buffers in the ring = images in flight (copy pending, queued or being written); threads: 1 or 2 writer threads.
    `open_fn(path, "wb")` opens the output (tests substitute it).  Seconds the caller spent blocked are accumulated in
    `wait_copy` (byte counts, i.e. the step) and `wait_writer` (no free slot / full queue)."""

    def __init__(self, slots=6, threads=2, open_fn=open):
        assert slots >= 1 and threads in (1, 2)
        self._open = open_fn
        self._jobs = queue.Queue(maxsize=slots)
        self._free = queue.Queue()
        for _ in range(slots):
            self._free.put(_Slot())
        self._error, self._lock, self._closed = None, threading.Lock(), False
        self.wait_copy, self.wait_writer, self.files, self.bytes = 0.0, 0.0, 0, 0
        self._threads = [threading.Thread(target=self._run, name="png-writer-%d" % i, daemon=True) for i in range(threads)]
        for t in self._threads:
            t.start()

    # ---- producer side ------------------------------------------------------------------------------------------------------
    def _check(self):
        if self._error is not None:
            raise self._error
        assert not self._closed, "PngWriter is closed"

    def _put(self, job):
        t0 = time.perf_counter()
        self._jobs.put(job)
        self.wait_writer += time.perf_counter() - t0

    def submit_bytes(self, path, stream, height, width):
        """queue a finished zlib stream that already lives in host memory (bytes-like); blocks while the queue is full"""
        self._check()
        self._put((path, stream, height, width, None, None))

    def submit(self, jobs):
        """jobs: [(path, stream, nbytes, H, W)] with `stream, nbytes` as `Ops.png_encode` returns them (device tensors, encode
        enqueued on the current stream).  Returns once the copies are enqueued; the tensors may be overwritten by work enqueued
        on that stream afterwards."""
        self._check()
        t0 = time.perf_counter()
        slots = [self._free.get() for _ in jobs]
        self.wait_writer += time.perf_counter() - t0
        for slot, (_, stream, nbytes, _, _) in zip(slots, jobs):
            slot.reserve(stream.numel())
            slot.count.copy_(nbytes.view(-1)[:1], non_blocking=True)
        counted = torch.cuda.Event()
        counted.record()
        t0 = time.perf_counter()
        counted.synchronize()
        self.wait_copy += time.perf_counter() - t0
        for slot, (path, stream, _, H, W) in zip(slots, jobs):
            n = int(slot.count[0])
            assert 0 < n <= stream.numel(), n
            slot.buf[:n].copy_(stream[:n], non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            self._put((path, slot.buf[:n].numpy(), H, W, done, slot))

    def close(self):
        """drain the queue, stop the threads, re-raise the first exception a worker met"""
        if not self._closed:
            self._closed = True
            for _ in self._threads:
                self._jobs.put(None)
            for t in self._threads:
                t.join()
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                       # do not mask the loop's own exception
            try:
                self.close()
            except Exception:
                pass
        return False

    # ---- writer threads -----------------------------------------------------------------------------------------------------
    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            path, stream, H, W, done, slot = job
            try:
                if self._error is None:             # after a failure the remaining jobs are only released
                    if done is not None:
                        done.synchronize()
                    parts = png_frame(stream, H, W)
                    with self._open(path, "wb") as fh:
                        for p in parts:
                            fh.write(p)
                    with self._lock:
                        self.files += 1
                        self.bytes += sum(len(p) for p in parts)
            except BaseException as e:              # noqa: BLE001 -- surfaced by close() / the next submit
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                if slot is not None:
                    self._free.put(slot)
