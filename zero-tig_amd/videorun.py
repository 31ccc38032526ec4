"""What the raw-video loops of predict.py, evals.py and train.py share: the WxH parser, the walk of a stream's sequences behind
the scene-cut detector, and the closing of a loop's writers and readers."""
import logging
import sys


def parse_size(text):
    """'WxH' -> (W, H), or None when it is not two positive integers"""
    parts = text.lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() and int(p) > 0 for p in parts):
        return None
    return int(parts[0]), int(parts[1])


class Sequences:
    """seq = Sequences(det, threshold, first=0, log=True); new_seq = seq.next(payload) once per frame, in stream order.

    `det`: a `SceneCut`, or None: the stream is one sequence and only frame 0 starts one.  The detector runs on a stream of its
    own; its copy of the payload has completed when `next` returns.  A cut the detector reports at frame 0 is not one: that frame
    starts a sequence anyway.  `first`: the stream index of the loop's frame 0 (a rank's share of a file), for `cuts` and the
    log line.  `cuts`: stream indices; `scores`, `rels`: the detector's two numbers of every frame; `flags`: per frame, whether it
    is a recorded cut."""

    def __init__(self, det, threshold, first=0, log=True):
        self.det, self.threshold, self.first, self.log = det, threshold, first, log
        self.cuts, self.scores, self.rels, self.flags = [], [], [], []

    def next(self, payload):
        i, cut = len(self.flags), False
        if self.det is not None:
            self.det.push(payload)
            is_cut, score, rel = self.det.pop()
            self.scores.append(score), self.rels.append(rel)
            cut = bool(is_cut) and i > 0
            if cut:
                self.cuts.append(self.first + i)
                if self.log:
                    logging.info("scene cut at frame %d: score %.4f (rel %.4f) > %g", self.first + i, score, rel, self.threshold)
        self.flags.append(cut)
        return cut or i == 0

    def cuts_json(self):
        return {"threshold": self.threshold, "cuts": self.cuts, "score": self.scores, "rel": self.rels}


def close_streams(writers, readers):
    """the `finally` of a video loop: every writer is drained and closed, then every reader (None entries are skipped); the first
    writer failure is the one reported, unless an exception is already on its way out of the loop"""
    errors = []
    for w in writers:
        if w is not None:
            try:
                w.close()
            except BaseException as e:             # noqa: BLE001
                errors.append(e)
    for r in readers:
        if r is not None:
            r.close()
    if errors and sys.exc_info()[0] is None:
        raise errors[0]
