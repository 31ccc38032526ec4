"""Temporal consistency of an enhanced video against its ground truth (evals.py --tc 1).

Per frame pair (t-1, t) of one sequence, at the reduced size (H // scale, W // scale):
  fb = RAFT(gt_t, gt_{t-1})   the backward flow, cur -> prev
  ff = RAFT(gt_{t-1}, gt_t)   the forward flow, prev -> cur
both from the GROUND TRUTH (they describe the scene's motion, not the result's artefacts), 12 iterations, `flow_up` at RAFT's padded
size; then `Ops.warp_error` (csrc/zt_temporal.hip) twice with those flows: on the output pair and on the ground-truth pair, whose
numbers are the floor the output's are read against.  Warping error: Lai et al. 2018 with the occlusion test of Ruder et al. 2016;
MABD: Jiang and Zheng 2019.  Nothing here synchronises with the device."""
import torch

from .lib import current_stream
from .raft import RaftPlan

# RAFT's correlation pyramid has four levels of the 1/8 map, each half the one before: the map must be at least 8 x 8
MIN_SIDE = 64
ITERS = 12


def too_small(H, W, scale):
    """-> why a frame of H x W cannot be graded at `scale`, or None"""
    h, w = H // scale, W // scale
    if min(h, w) < MIN_SIDE:
        return "the reduced frame is %dx%d, RAFT's four-level pyramid needs %d pixels a side" % (w, h, MIN_SIDE)
    return None


def load_raft_weights(path, like, dev):
    """a RAFT state dict in the reference's key names (`fnet.conv1.weight`, ...; a `module.` prefix, as DataParallel leaves it, and a
    `raft.` prefix are accepted) -> {"raft." + name: fp32 tensor on dev}.  `like`: the state dict of the model's own RAFT, which
    fixes the names and shapes; a missing tensor or another shape raises ValueError."""
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
        sd = sd["state_dict"]
    got = {}
    for k, v in sd.items():
        k = k[7:] if k.startswith("module.") else k
        k = k[5:] if k.startswith("raft.") else k
        got[k] = v
    out = {}
    for k, ref in like.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k not in got:
            raise ValueError("%s: no tensor %r (a RAFT-basic state dict in the reference's key names is expected)" % (path, k))
        if tuple(got[k].shape) != tuple(ref.shape):
            raise ValueError("%s: %r is %s, RAFT-basic has %s" % (path, k, tuple(got[k].shape), tuple(ref.shape)))
        out["raft." + k] = got[k].detach().to(device=dev, dtype=torch.float32).contiguous()
    return out


class TemporalConsistency:
    """tc = TemporalConsistency(ops, raft_weights, dev, H, W, scale, precision)
       tc.reset()                                   # a new sequence: the next frame has no partner
       tc.push(output, gt, ri, rf) -> bool          # True when a pair was graded

    `raft_weights`: {"raft.*": tensor on dev}.  The RAFT plan is this object's own; it shares nothing with the plan inside a captured
    `InferStep` graph, and it runs on the current stream alone: the grading stays strictly in stream order between two replays of
    the step's graph, at the price of the context encoder's overlap (about 0.1 ms a call, raft.py).
    `output`, `gt`: fp32 [1,3,H,W] in [0, 1]; both are reduced (or, at scale 1, copied: the step's output buffer is overwritten by the
    next frame) before `push` returns to the caller's stream order.
    `ri`: int64 [2], `rf`: float64 [6] on the device, e.g. slices of a table row: ri[0], rf[0:3] = `Ops.warp_error` of the output
    pair, ri[1], rf[3:6] = of the ground-truth pair.  The first frame after `reset()` writes nothing.
    `fb`, `ff`: the flows last used ([1,2,Hp,Wp], the padded size).
    `keep_pair=True` keeps the reduced frames of the last push (and of its partner), so that `viz` can draw them:
       tc.viz(out, which="out", radius=0.0, gain=4.0)   # the four-panel picture of the last pushed frame into out [1,3,2h,2w]
    `push` and its numbers are the same either way.
    `alternate_corr=True`: both RAFT runs look their correlation up from the feature maps and form no all-pairs volume."""

    def __init__(self, ops, raft_weights, dev, H, W, scale, precision, keep_pair=False, alternate_corr=False):
        why = too_small(H, W, scale)
        if why is not None or scale < 1:
            raise ValueError("TemporalConsistency: scale %d at %dx%d: %s" % (scale, W, H, why or "the scale is an integer >= 1"))
        self.ops, self.dev, self.H, self.W, self.scale = ops, dev, int(H), int(W), int(scale)
        self.h, self.w = self.H // self.scale, self.W // self.scale
        self.Hp, self.Wp = (self.h + 7) // 8 * 8, (self.w + 7) // 8 * 8
        self.plan = RaftPlan(ops, raft_weights, dev, precision=precision, alternate_corr=alternate_corr)
        self.plan.two_streams = False
        self.fb = self.ff = None
        self.pairs = 0
        self.keep_pair = bool(keep_pair)
        self._last = None                          # keep_pair: (cur, prev or None) of the last push
        self._radius = torch.empty(1, dtype=torch.float32, device=dev) if keep_pair else None
        self.reset()

    def reset(self):
        self._prev = None                          # (output, gt, gt * 255) of the previous frame, reduced

    def _reduced(self, x, mul):
        if self.scale == 1 and mul == 1.0:
            return x.detach().clone()
        return self.ops.resize_bilinear(x, self.h, self.w, mul)

    def flow(self, img1, img2):
        """RAFT(img1, img2): the flow from img1 to img2 in pixels; frames [1,3,h,w] in [0, 255] -> [1,2,Hp,Wp]"""
        p = self.plan
        x2 = torch.empty((2, self.Hp, self.Wp, 8 if p.h else 4), dtype=p.adt, device=self.dev)
        self.ops.lib.call("zt_raft_pack_pair", img1, img2, x2, p.dt, x2.shape[-1], self.h, self.w, self.Hp, self.Wp, current_stream(self.dev))
        return p.run(x2, iters=ITERS)[1]

    def push(self, output, gt, ri, rf):
        assert tuple(output.shape) == (1, 3, self.H, self.W) and output.shape == gt.shape, (output.shape, gt.shape)
        assert tuple(ri.shape) == (2,) and tuple(rf.shape) == (6,), (ri.shape, rf.shape)
        output, gt = output.contiguous(), gt.contiguous()
        cur = (self._reduced(output, 1.0), self._reduced(gt, 1.0), self.ops.resize_bilinear(gt, self.h, self.w, 255.0))
        prev, self._prev = self._prev, cur
        if self.keep_pair:
            self._last = (cur, prev)
        if prev is None:
            return False
        self.fb = self.flow(cur[2], prev[2])
        self.ff = self.flow(prev[2], cur[2])
        self.ops.warp_error(cur[0], prev[0], self.fb, self.ff, out_n=ri[0:1], out3=rf[0:3])
        self.ops.warp_error(cur[1], prev[1], self.fb, self.ff, out_n=ri[1:2], out3=rf[3:6])
        self.pairs += 1
        return True

    def viz(self, out, which="out", radius=0.0, gain=4.0):
        """the picture of `Ops.tc_viz` for the frame last pushed, into `out` (fp32 [1,3,2h,2w]): of the pair when that push
        returned True, of the frame alone (white flow panels, no flags, no error) otherwise.  `which`: "out" draws the output
        pair, "gt" the ground-truth pair, both against the flows the numbers were taken with.  `radius` > 0: the flow length in
        reduced-frame pixels that is drawn at full saturation; 0: the larger of the two flows' largest radii, per pair.
        Nothing synchronises."""
        assert self.keep_pair and self._last is not None, "viz needs keep_pair=True and a pushed frame"
        assert which in ("out", "gt") and radius >= 0 and gain >= 0, (which, radius, gain)
        cur, prev = self._last
        k = 0 if which == "out" else 1
        if prev is None:
            return self.ops.tc_viz(cur[k], None, None, None, None, gain, out=out)
        if radius > 0:
            self._radius.fill_(float(radius))
        else:
            self.ops.flow_radmax(self.fb, self.ff, h=self.h, w=self.w, out=self._radius)
        return self.ops.tc_viz(cur[k], prev[k], self.fb, self.ff, self._radius, gain, out=out)
