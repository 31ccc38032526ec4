"""zt_warp_error_f32 (csrc/zt_temporal.hip) against a numpy float32 restatement of its definition, on the host emulator
and, under -m gpu, on the MI355X.

Gates and where they come from:
* out_n: equal.  Every per-pixel value is IEEE fp32 with one rounding per operation on both sides (no fused multiply-add in the
  kernel, none in numpy), so the mask is the same mask.
* the three sums: relative 1e-9 (absolute 1e-9 * 1 where the reference is 0: then ours must be 0 too, see `_close`).  The terms are
  bit-identical, each is converted to double before it is added, so only the order of at most 136 * 200 = 2.7e4 fp64 additions
  differs: n * 2^-53 = 3e-12.  1e-9 is SSIM_TOL, the project's gate for fp64 reductions.
* a second call returns the same bits.

The flow kinds make the mask work: `_smooth` is tuned so that, asserted on the restatement alone, between 20 % and 80 % of the
pixels that land inside the frame pass the forward-backward test and at least 2 % land outside (sizes of one pixel cannot show a
share, they run without that assertion).  `_planted` puts NaN, +inf, 1e30 and -1e30 into both flows: by the definition a pixel
whose own backward flow is one of them lands outside the frame and is invalid; a pixel that only READS such a forward flow through
its bilinear taps is invalid for NaN, while +-1e30 and inf overflow both sides of the test to +inf, and inf <= inf holds -- the
restatement and the kernel agree on that, it is recorded in DESIGN 8i.  No pixel that reads no planted value changes, and every
output stays finite because no planted value reaches an address or an image term."""
import numpy as np
import pytest
import torch

from test_metrics import SSIM_TOL

F = np.float32
# (H, W, Hf, Wf): 1 x 1; 5 x 7; 38 x 52: tails in both axes, value-wide loads; 33 x 130 inside 40 x 136 (oy, ox = 3, 3); 136 x 200:
# 16-byte loads, 34 tiles = more than one block and more than one partial.  16 x 64 inside 24 x 72 (ox = 4: 16-byte loads of the
# flows behind an offset) and inside 24 x 70 (ox = 3: 16-byte loads of the images only) are the two mixed paths
SIZES = [(1, 1, 1, 1), (5, 7, 5, 7), (38, 52, 38, 52), (33, 130, 40, 136), (136, 200, 136, 200), (16, 64, 24, 72), (16, 64, 24, 70)]
KINDS = ["zero", "shift", "half", "smooth", "planted"]
SHIFT = 3


def restate(cur, prev, fb, ff, oy, ox):
    """the definition of DESIGN 8i in numpy float32 -> (n, [sum e over valid, sum e0, sum b], valid mask, e, inside mask)"""
    _, H, W = cur.shape
    assert all(a.dtype == F for a in (cur, prev, fb, ff))
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    win = (slice(oy, oy + H), slice(ox, ox + W))             # every tap lies in [0, H - 1] x [0, W - 1] of this window
    u, v = fb[0][win], fb[1][win]
    with np.errstate(all="ignore"):
        px, py = xs.astype(F) + u, ys.astype(F) + v
        inside = (px >= F(0)) & (px <= F(W - 1)) & (py >= F(0)) & (py <= F(H - 1))
        px, py = np.where(inside, px, F(0)), np.where(inside, py, F(0))
        fx0, fy0 = np.floor(px), np.floor(py)
        ax, ay = px - fx0, py - fy0
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)

        def bil(p):
            top = (F(1) - ax) * p[y0, x0] + ax * p[y0, x1]
            bot = (F(1) - ax) * p[y1, x0] + ax * p[y1, x1]
            return (F(1) - ay) * top + ay * bot
        fu, fv = bil(ff[0][win]), bil(ff[1][win])
        su, sv = u + fu, v + fv
        lhs = su * su + sv * sv
        rhs = F(0.01) * ((u * u + v * v) + (fu * fu + fv * fv)) + F(0.5)
        valid = inside & (lhs <= rhs)
        d = [cur[c] - bil(prev[c]) for c in range(3)]
        e = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        s = [cur[c] - prev[c] for c in range(3)]
        e0 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        b = np.abs(((cur[0] + cur[1]) + cur[2]) - ((prev[0] + prev[1]) + prev[2]))
    assert all(a.dtype == F for a in (px, ax, fu, lhs, rhs, e, e0, b))
    sums = [float(e[valid].astype(np.float64).sum()), float(e0.astype(np.float64).sum()), float(b.astype(np.float64).sum())]
    return int(valid.sum()), sums, valid, e, inside


def _smooth(rng, H, W, amp):
    """two smooth planes [2][H][W]: a few low-frequency waves with random phases, peak about `amp` pixels"""
    ys, xs = np.meshgrid(np.arange(H) / max(H, 8), np.arange(W) / max(W, 8), indexing="ij")
    out = np.zeros((2, H, W))
    for c in range(2):
        for _ in range(3):
            ky, kx = rng.uniform(-1.5, 1.5, 2)
            out[c] += np.sin(2 * np.pi * (ky * ys + kx * xs) + rng.uniform(0, 2 * np.pi))
    return (amp / 2.0 * out).astype(F)


# amplitudes of the smooth kind, tuned on the restatement alone: the backward flow peaks at 12 % of the shorter side, at least 1 and
# at most 6 pixels, so that a few per cent of the pixels leave the frame at every size; the noise on the forward flow peaks at 0.8
# pixels, around the test's threshold of sqrt(0.5 + 0.01 (|fb|^2 + |ff|^2)).  Shares these give: 26 % .. 74 % valid, 3.7 % .. 51 %
# outside.
def _amps(H, W):
    return min(6.0, max(1.0, 0.12 * min(H, W))), 0.8


_CASES = {}


def _case(kind, size):
    """(cur, prev, fb, ff, oy, ox, restatement) -- made once, never modified"""
    key = (kind, size)
    if key in _CASES:
        return _CASES[key]
    H, W, Hf, Wf = size
    oy, ox = (Hf - H) // 2, (Wf - W) // 2
    rng = np.random.default_rng(1000 * H + W + 7 * Hf + Wf)
    prev = rng.random((3, H, W), dtype=F)
    cur = rng.random((3, H, W), dtype=F)
    # outside the frame's window the padded flows hold values that would show up if they were read for the wrong pixel
    fb, ff = (rng.uniform(-50, 50, (2, Hf, Wf)).astype(F) for _ in range(2))
    win = (slice(None), slice(oy, oy + H), slice(ox, ox + W))
    if kind == "zero":
        fb[win], ff[win] = 0, 0
    elif kind == "shift":                                   # cur(x) = prev(x - SHIFT): backward flow -SHIFT, forward flow +SHIFT
        fb[win], ff[win] = 0, 0
        fb[0][win[1:]], ff[0][win[1:]] = -SHIFT, SHIFT
        cur[:, :, SHIFT:] = prev[:, :, :max(W - SHIFT, 0)]
    elif kind == "half":
        fb[win], ff[win] = 0, 0
        fb[0][win[1:]], ff[0][win[1:]] = 0.5, -0.5
    else:
        a_flow, a_noise = _amps(H, W)
        f = _smooth(rng, H, W, a_flow)
        fb[win] = f
        ff[win] = -f + _smooth(rng, H, W, a_noise)
        if kind == "planted":
            bad = [np.nan, np.inf, 1e30, -1e30]
            pos = rng.permutation(H * W)
            for i, val in enumerate(bad):
                for j, flow in enumerate((fb, ff)):
                    q = int(pos[(2 * i + j) % pos.size])     # eight places when the frame has them
                    flow[i % 2, oy + q // W, ox + q % W] = val
    for a in (cur, prev, fb, ff):
        a.setflags(write=False)
    _CASES[key] = (cur, prev, fb, ff, oy, ox, restate(cur, prev, fb, ff, oy, ox))
    return _CASES[key]


def _place(a, dev, offset=0):
    """`a` in a fresh buffer on `dev`, `offset` floats behind a 16-byte aligned address, as a [1, C, H, W] tensor"""
    buf = torch.zeros(a.size + offset + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + a.size].view((1,) + a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    return view


def _close(ours, ref):
    return abs(ours - ref) <= SSIM_TOL * abs(ref) if ref != 0.0 else ours == 0.0


def _run(ops, dev, case, offset=0):
    cur, prev, fb, ff = (_place(a, dev, offset) for a in case[:4])
    n, s = ops.warp_error(cur, prev, fb, ff)
    assert n.dtype == torch.int64 and s.dtype == torch.float64 and n.device.type == dev.type and s.device.type == dev.type
    n2, s2 = ops.warp_error(cur, prev, fb, ff)              # the same bits again (and a reused workspace)
    assert n.tolist() == n2.tolist() and s.numpy(force=True).tobytes() == s2.numpy(force=True).tobytes()
    return int(n.item()), s.tolist()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-in-%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_warp_error_parity(backend, kind, size):
    ops, dev, _ = backend
    H, W = size[:2]
    case = _case(kind, size)
    n_ref, s_ref, valid, e, inside = case[6]
    # ---- what the case must exercise, asserted on the restatement alone
    if kind == "zero":
        assert n_ref == H * W and s_ref[0] == s_ref[1] > 0
    elif kind == "shift":
        assert n_ref == H * max(W - SHIFT, 0) and s_ref[0] == 0.0 and (e[valid] == 0).all()
    elif kind == "half":
        assert n_ref == H * (W - 1) and (s_ref[0] > 0 or W == 1)
    elif H * W > 1:
        n_in = int(inside.sum())
        assert H * W - n_in >= 0.02 * H * W, (n_in, H * W)
        assert 0.2 * n_in <= n_ref <= 0.8 * n_in, (n_ref, n_in)
    assert all(np.isfinite(v) for v in s_ref)
    # ---- the kernel against it
    n, s = _run(ops, dev, case)
    print("warp_error %s %s: n %d ref %d, sums %r ref %r" % (kind, size, n, n_ref, s, s_ref))
    assert n == n_ref
    assert all(_close(a, b) for a, b in zip(s, s_ref)), (s, s_ref)
    if kind == "zero":
        assert s[0] == s[1]
    if kind == "shift":
        assert s[0] == 0.0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-in-%dx%d" % s)
def test_planted_values_touch_only_their_readers(size):
    """on the restatement: a pixel whose backward flow is NaN, inf or +-1e30 is invalid; a pixel that reads no planted value keeps
    its mask bit and its error"""
    H, W, Hf, Wf = size
    cur, prev, fb, ff, oy, ox, (n, s, valid, e, inside) = _case("planted", size)
    _, _, fb0, ff0, _, _, (n0, s0, valid0, e0, inside0) = _case("smooth", size)
    win = (slice(oy, oy + H), slice(ox, ox + W))
    own = np.zeros((H, W), bool)                             # pixels whose own backward flow was planted
    for c in range(2):
        own |= ~(fb[c][win] == fb0[c][win])
    assert own.any() and not valid[own].any() and not inside[own].any()
    hit = np.zeros((H, W), bool)                             # planted samples of the forward flow
    for c in range(2):
        hit |= ~(ff[c][win] == ff0[c][win])
    assert hit.any()
    # readers: the four taps of every pixel, taken from the unplanted case (an unplanted pixel has the same taps in both)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        px = np.where(inside0, xs.astype(F) + fb0[0][win], F(0))
        py = np.where(inside0, ys.astype(F) + fb0[1][win], F(0))
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    reads = hit[y0, x0] | hit[y0, x1] | hit[y1, x0] | hit[y1, x1]
    rest = ~(own | reads)
    assert (valid[rest] == valid0[rest]).all() and (e[rest] == e0[rest]).all() and (inside[rest] == inside0[rest]).all()
    assert np.isfinite(e).all() and all(np.isfinite(v) for v in s)


@pytest.mark.parametrize("kind", ["smooth", "planted"])
def test_warp_error_unaligned_pointers(backend, kind):
    """136 x 200 takes the 16-byte loads from aligned buffers; one float further on the same values take the value-wide loads"""
    ops, dev, _ = backend
    case = _case(kind, (136, 200, 136, 200))
    n_ref, s_ref = case[6][:2]
    n, s = _run(ops, dev, case, offset=1)
    assert n == n_ref and all(_close(a, b) for a, b in zip(s, s_ref)), (n, n_ref, s, s_ref)
    assert (n, s) == _run(ops, dev, case)                   # the same pixels in the same order: the same bits


def test_warp_error_out_slices(backend):
    ops, dev, _ = backend
    case = _case("smooth", (38, 52, 38, 52))
    cur, prev, fb, ff = (_place(a, dev) for a in case[:4])
    n, s = ops.warp_error(cur, prev, fb, ff)
    ri = torch.full((4,), -1, dtype=torch.int64, device=dev)
    rf = torch.full((6,), -1.0, dtype=torch.float64, device=dev)
    ops.warp_error(cur, prev, fb, ff, out_n=ri[2:3], out3=rf[1:4])
    assert ri.tolist() == [-1, -1, int(n.item()), -1]
    assert rf.tolist() == [-1.0] + s.tolist() + [-1.0, -1.0]


def test_warp_error_argument_errors(backend):
    ops, dev, _ = backend
    img = torch.zeros(3 * 8 * 8, dtype=torch.float32, device=dev)
    flow = torch.zeros(2 * 16 * 16, dtype=torch.float32, device=dev)
    ws = torch.zeros(4 * 4, dtype=torch.int64, device=dev)
    n, s = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)

    def call(cur=img, prev=img, fb=flow, ff=flow, H=8, W=8, Hf=16, Wf=16, oy=4, ox=4, w=ws, nblk=4, on=n, o3=s):
        ops.lib.call("zt_warp_error_f32", cur, prev, fb, ff, H, W, Hf, Wf, oy, ox, w, nblk, on, o3, None)
    call()                                                                       # the well-formed call
    assert n.tolist() == [64] and s.tolist() == [0.0, 0.0, 0.0]
    bad = [{"Hf": 11}, {"Wf": 11}, {"oy": 9}, {"ox": 9}, {"oy": -1}, {"ox": -1}, {"H": 0}, {"W": 0}, {"H": -8}, {"nblk": 0},
           {"nblk": -1}, {"nblk": 4097}, {"cur": None}, {"prev": None}, {"fb": None}, {"ff": None}, {"w": None}, {"on": None},
           {"o3": None}]
    for kw in bad:
        with pytest.raises(RuntimeError, match="1001"):
            call(**kw)
    with pytest.raises(AssertionError):                                          # the wrapper checks the shapes
        ops.warp_error(img.view(1, 3, 8, 8), img.view(1, 3, 8, 8), flow[:72].view(1, 2, 6, 6), flow[:72].view(1, 2, 6, 6))
