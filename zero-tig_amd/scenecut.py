"""Scene cuts in a raw video stream (`predict.py --y4m_scene_cut`): where a Y4M stream starts a new sequence.

The decision needs the input luma of two consecutive frames and nothing of the model, so it is made ahead of the step on a stream of
its own; `pop` waits for the detector's event, never for the device or the step's stream.  (Measured in DESIGN 8e: in a device-bound
loop that event still completes about a frame late, so the host stops running ahead of the device and the loop loses 4 %.)

The score.  The luma plane is cut into 16 x 16 cells (edge cells hold the pixels that exist); G[i][j] = sum over the cell of
max(Y - yo, 0), yo = 16 for limited range and 0 for full range (`Ops.luma_grid`; a deep stream's luma is first cut to its top 8
bits, so a threshold means the same at every depth).  For a pair of frames sad = sum |G_n - G_(n-1)|
and tot = sum (G_n + G_(n-1)), 64-bit integers (`Ops.grid_sad`).  On the host rel_n = sad / max(tot, 1), rel_0 = 0,
score_n = min(rel_n, |rel_n - rel_(n-1)|), and frame n starts a sequence when score_n > threshold; frame 0 always does."""
import time

import torch


class CutRule:
    """The host side of the score: keeps rel_(n-1), nothing else."""

    def __init__(self, threshold):
        self.threshold, self.rel = float(threshold), None

    def first(self):
        self.rel = 0.0
        return True, 0.0, 0.0

    def update(self, sad, tot):
        """(sad, tot) of frames n - 1 and n -> (is_cut, score, rel)"""
        rel = int(sad) / max(int(tot), 1)
        score = min(rel, abs(rel - self.rel))
        self.rel = rel
        return score > self.threshold, score, rel


class SceneCut:
    """det = SceneCut(ops, dev, fmt, threshold); per frame det.push(payload), then is_cut, score, rel = det.pop().

    `push` takes the frame's payload (1-D uint8 of `fmt`, pinned host memory or on the device) and, on the detector's own stream,
    copies its luma plane into one of two device slots, makes the grid, compares it with the previous frame's and copies the pair
    to pinned host memory; an event follows.  `pop` waits for that event only -- the copy out of `payload` has completed when it
    returns -- and applies the host rule.  Frame 0 gives (True, 0.0, 0.0).  On a CPU device (the test emulator) the same calls run
    synchronously.  `wait` accumulates the seconds `pop` spent blocked."""

    def __init__(self, ops, dev, fmt, threshold):
        fmt.check()
        self.ops, self.dev, self.fmt, self.rule = ops, torch.device(dev), fmt, CutRule(threshold)
        self._n = fmt.H * fmt.W * (2 if fmt.depth > 8 else 1)      # the luma plane's bytes
        cells = ((fmt.H + 15) // 16) * ((fmt.W + 15) // 16)
        self._cuda = self.dev.type == "cuda"
        self._stream = torch.cuda.Stream(self.dev) if self._cuda else None
        self._luma = [torch.empty(self._n, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self._grid = [torch.empty(cells, dtype=torch.int32, device=self.dev) for _ in range(2)]
        self._pair = torch.empty(2, dtype=torch.int64, device=self.dev)
        self._host = torch.zeros(2, dtype=torch.int64, pin_memory=self._cuda)
        self._event, self._pending = None, False
        self.frames, self.wait = 0, 0.0

    def _enqueue(self, payload):
        k = self.frames & 1
        self._luma[k].copy_(payload[:self._n], non_blocking=True)
        self.ops.luma_grid(self._luma[k], self.fmt, out=self._grid[k])
        if self.frames:
            self.ops.grid_sad(self._grid[k], self._grid[k ^ 1], out=self._pair)
            self._host.copy_(self._pair, non_blocking=True)

    def push(self, payload):
        assert not self._pending, "SceneCut.push: pop() the previous frame first"
        assert payload.dtype == torch.uint8 and payload.dim() == 1 and payload.numel() == self.fmt.frame_bytes, \
            (payload.dtype, tuple(payload.shape), self.fmt.frame_bytes)
        if self._cuda:
            if payload.device.type == "cuda":                # made on the caller's stream: the copy is ordered behind it
                self._stream.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(self._stream):
                self._enqueue(payload)
                self._event = torch.cuda.Event()
                self._event.record()
        else:
            self._enqueue(payload)
        self._pending = True

    def pop(self):
        assert self._pending, "SceneCut.pop: nothing was pushed"
        if self._event is not None:
            t0 = time.perf_counter()
            self._event.synchronize()
            self.wait += time.perf_counter() - t0
        self._pending = False
        self.frames += 1
        if self.frames == 1:
            return self.rule.first()
        return self.rule.update(int(self._host[0]), int(self._host[1]))
