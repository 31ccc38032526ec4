"""Plane metrics of two raw video payloads on the device (csrc/zt_planes.hip): zt_yuv_sse and zt_ssim_plane.

Gates and where they come from:
* zt_yuv_sse: bit for bit against numpy int64 on the clamped planes, no tolerance.
* zt_ssim_plane: |ours - ref| <= SSIM_TOL (1e-9, tests/test_metrics.py).  The reference is the formula of `ssim_ref` there for one
  plane with data_range = m = 2^depth - 1; its five window sums are exact integers (an int64 summed-area table) before they go to
  float64, so it carries no filter rounding at 16 bits, where 49 * 65535^2 = 2^37.6 still sits far below 2^53.  What is left on
  both sides is a few dozen fp64 operations per window and the order of the final mean: 1e-16 .. 1e-15 (figures in DESIGN 8h)."""
import importlib

import numpy as np
import pytest
import torch

from test_metrics import SSIM_TOL

DEEP = (9, 10, 12, 14, 16)


def _y4m():
    return importlib.import_module("zero-tig_amd.y4m")


def _fmt(H, W, ss, depth):
    return _y4m().YuvFormat(W, H, ss, 0 if ss == 444 else 1, "bt709", 0, depth)


def _place(payload, dev, offset=0):
    """the bytes of `payload` in a fresh buffer on `dev`, `offset` bytes behind a 16-byte aligned address"""
    p = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    buf = torch.zeros(p.size + offset + 16, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + p.size]
    view.copy_(torch.from_numpy(p.copy()))
    return view


def _samples(rng, n, depth, over=True):
    """n random samples of `depth` bits as the payload stores them; a deep payload also holds samples above m (read as m)"""
    if depth == 8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    m = (1 << depth) - 1
    v = rng.integers(0, m + 1, n).astype("<u2")
    if over and depth < 16 and n >= 4:
        idx = rng.permutation(n)[:max(1, n // 8)]
        v[idx] = rng.integers(m + 1, 65536, idx.size).astype("<u2")
        v[idx[0]] = 65535
    return v


def _clamped_planes(fmt, payload):
    m = (1 << fmt.depth) - 1
    return [np.minimum(p.astype(np.int64), m) for p in fmt.planes(np.ascontiguousarray(payload).view(np.uint8))]


# ================================================================= zt_yuv_sse ===============================================
def sse_ref(fmt, pa, pb):
    return [int(((x - y) ** 2).sum()) for x, y in zip(_clamped_planes(fmt, pa), _clamped_planes(fmt, pb))]


# the sizes of tests/test_y4m.py (2 x 2: one chroma sample; 38 x 52 and 6 x 258: tails in both axes, sample-wide loads; 24 x 200:
# 16-byte loads at 16 bits) and 24 x 208, the 16-byte path at 8 bits (W % 16 == 0)
SSE_SIZES = [(2, 2), (38, 52), (6, 258), (24, 200), (24, 208)]


@pytest.mark.parametrize("size", SSE_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ss", [420, 422, 444])
@pytest.mark.parametrize("depth", [8, 10, 16])
def test_sse_exact(backend, depth, ss, size):
    ops, dev, _ = backend
    H, W = size
    fmt = _fmt(H, W, ss, depth)
    n = fmt.frame_bytes // (2 if depth > 8 else 1)
    rng = np.random.default_rng(depth * 100000 + ss * 100 + H + W)
    pa, pb = _samples(rng, n, depth), _samples(rng, n, depth)
    ref = sse_ref(fmt, pa, pb)
    assert all(v > 0 for v in ref)
    da, db = _place(pa, dev), _place(pb, dev)
    got = ops.yuv_sse(da, db, fmt)
    assert got.dtype == torch.int64 and got.device.type == dev.type and got.tolist() == ref
    assert ops.yuv_sse(da, db, fmt).tolist() == ref                              # the same bits again (and a reused workspace)
    # one sample behind an aligned address: the sample-wide loads, the same integers
    es = 2 if depth > 8 else 1
    assert ops.yuv_sse(_place(pa, dev, es), _place(pb, dev, es), fmt).tolist() == ref
    assert ops.yuv_sse(da, _place(pb, dev, es), fmt).tolist() == ref
    assert ops.yuv_sse(da, _place(pa, dev), fmt).tolist() == [0, 0, 0]
    row = torch.full((5,), -1, dtype=torch.int64, device=dev)                   # out=: a slice of a table row
    ops.yuv_sse(da, db, fmt, out=row[1:4])
    assert row.tolist() == [-1] + ref + [-1]


@pytest.mark.parametrize("ss", [420, 444])
def test_sse_saturated_16bit(backend, ss):
    """a = 0 against b = 65535 everywhere: every partial is far above 2^32 (1976 * 65535^2 = 2^42.9 for the luma plane)"""
    ops, dev, _ = backend
    fmt = _fmt(38, 52, ss, 16)
    n = fmt.frame_bytes // 2
    pa, pb = np.zeros(n, "<u2"), np.full(n, 65535, "<u2")
    hc, wc = fmt.chroma_shape
    ref = [65535 ** 2 * k for k in (38 * 52, hc * wc, hc * wc)]
    assert ref[0] > 2 ** 32 and sse_ref(fmt, pa, pb) == ref
    assert ops.yuv_sse(_place(pa, dev), _place(pb, dev), fmt).tolist() == ref
    assert ops.yuv_sse(_place(pb, dev, 2), _place(pa, dev, 2), fmt).tolist() == ref


def test_sse_clamp_is_part_of_the_definition(backend):
    """10 bits: 65535 and 1023 are the same sample, 1024 and 1022 differ by one"""
    ops, dev, _ = backend
    fmt = _fmt(2, 8, 444, 10)
    pa, pb = np.full(48, 65535, "<u2"), np.full(48, 1023, "<u2")
    assert ops.yuv_sse(_place(pa, dev), _place(pb, dev), fmt).tolist() == [0, 0, 0]
    pa[:], pb[:] = 1024, 1022
    assert ops.yuv_sse(_place(pa, dev), _place(pb, dev), fmt).tolist() == [16, 16, 16]


def test_sse_argument_errors(backend):
    ops, dev, _ = backend
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    part, out = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

    def call(a, b, H, W, ss, depth, partial=part, nblk=1, o=out):
        ops.lib.call("zt_yuv_sse", a, b, H, W, ss, depth, partial, nblk, o, None)
    call(buf, buf, 8, 8, 420, 8)                                                 # the well-formed call
    bad = [(buf, buf, 8, 7, 420, 8), (buf, buf, 7, 8, 420, 8), (buf, buf, 8, 7, 422, 8), (buf, buf, 8, 8, 411, 8),
           (buf, buf, 0, 8, 444, 8), (buf, buf, 8, -8, 444, 8), (None, buf, 8, 8, 444, 8), (buf, None, 8, 8, 444, 8)]
    bad += [(buf, buf, 8, 8, 444, d) for d in (0, 7, 11, 13, 15, 17, 32)]
    for args in bad:
        with pytest.raises(RuntimeError, match="1001"):
            call(*args)
    for kw in ({"partial": None}, {"o": None}, {"nblk": 0}, {"nblk": 4097}):
        with pytest.raises(RuntimeError, match="1001"):
            call(buf, buf, 8, 8, 444, 8, **kw)
    with pytest.raises(RuntimeError, match="1001"):                              # a 16-bit sample at an odd address
        call(buf[1:], buf, 8, 8, 444, 16)
    with pytest.raises(RuntimeError, match="1001"):                              # 2^31 samples: the bound of the 64-bit sums
        call(buf, buf, 1 << 16, 1 << 15, 444, 8)
    with pytest.raises(AssertionError):                                          # the wrapper checks the payload's length
        ops.yuv_sse(buf[:100], buf[:100], _fmt(8, 8, 444, 8))


# ================================================================= zt_ssim_plane ============================================
def ssim_plane_ref(a, b, m):
    """skimage.metrics.structural_similarity(a, b, data_range=m) of two 2-D integer planes (gaussian_weights=False): the formula of
    tests/test_metrics.py:ssim_ref for one channel, the 7 x 7 window sums taken from int64 summed-area tables (exact)."""
    a, b = np.minimum(a.astype(np.int64), m), np.minimum(b.astype(np.int64), m)
    H, W = a.shape

    def win(x):
        c = np.zeros((H + 1, W + 1), dtype=np.int64)
        c[1:, 1:] = x.cumsum(axis=0).cumsum(axis=1)
        return (c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]).astype(np.float64)
    C1, C2 = (0.01 * m) ** 2, (0.03 * m) ** 2
    cov_norm = 49.0 / 48.0
    ux, uy = win(a) / 49.0, win(b) / 49.0
    uxx, uyy, uxy = win(a * a) / 49.0, win(b * b) / 49.0, win(a * b) / 49.0
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    assert S.shape == (H - 6, W - 6)
    return float(S.mean(dtype=np.float64))


def _backend_size_cases(small, large):
    out = [pytest.param("emu", s, id="emu-%dx%d" % s) for s in small]
    return out + [pytest.param("hip", s, id="hip-%dx%d" % s, marks=pytest.mark.gpu) for s in list(small) + list(large)]


SSIM_CASES = _backend_size_cases([(7, 7), (30, 44), (37, 53)], [(270, 480)])
_PAIRS = {}


def _plane_pair(kind, depth, H, W):
    """two planes as the payload stores them -- made once, never modified"""
    key = (kind, depth, H, W)
    if key not in _PAIRS:
        rng = np.random.default_rng(depth * 1000003 + H * 1009 + W)
        m = (1 << depth) - 1
        dt = np.uint8 if depth == 8 else np.dtype("<u2")
        if kind == "random":
            a, b = _samples(rng, H * W, depth), _samples(rng, H * W, depth)
        elif kind == "self":
            a = _samples(rng, H * W, depth)
            b = a.copy()
        elif kind == "const":
            a, b = np.full(H * W, int(0.3 * m), dt), np.full(H * W, int(0.7 * m), dt)
        else:
            assert kind == "dark"                           # a dark ramp, one of the pair with noise: what a low-light clip looks like
            ramp = (np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) * (0.08 * m / (W + 2 * H))
            a = np.round(ramp).astype(dt).reshape(-1)
            b = np.clip(np.round(ramp + rng.normal(0.0, 0.01 * m, (H, W))), 0, m).astype(dt).reshape(-1)
        a, b = a.reshape(H, W), b.reshape(H, W)
        a.setflags(write=False), b.setflags(write=False)
        _PAIRS[key] = (a, b, ssim_plane_ref(a, b, m))
    return _PAIRS[key]


def _payloads444(a, b):
    """two 4:4:4 payloads whose planes are (a, b, a) and (b, a, a): plane 0 grades a against b, plane 1 b against a from a plane
    pointer inside the payload (unaligned whenever H * W is odd), plane 2 a plane against itself"""
    return np.concatenate([a.reshape(-1), b.reshape(-1), a.reshape(-1)]), np.concatenate([b.reshape(-1), a.reshape(-1), a.reshape(-1)])


@pytest.mark.parametrize("kind", ["random", "self", "const", "dark"])
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("backend,size", SSIM_CASES, indirect=["backend"])
def test_ssim_plane_parity(backend, size, depth, kind):
    ops, dev, _ = backend
    H, W = size
    a, b, ref = _plane_pair(kind, depth, H, W)
    fmt = _fmt(H, W, 444, depth)
    pa, pb = (_place(p, dev) for p in _payloads444(a, b))
    got = [ops.ssim_plane(pa, pb, fmt, p) for p in range(3)]
    assert all(g.dtype == torch.float64 and g.numel() == 1 and g.device.type == dev.type for g in got)
    ours, swapped, same = (float(g.item()) for g in got)
    print("ssim_plane %s %d-bit %dx%d: ours %.17g ref %.17g |d| %.3g" % (kind, depth, H, W, ours, ref, abs(ours - ref)))
    assert abs(ours - ref) <= SSIM_TOL, (ours, ref)
    assert abs(swapped - ref) <= SSIM_TOL, (swapped, ref)
    assert same == 1.0
    if kind == "self":
        assert ours == 1.0 and ref == 1.0
    else:
        assert ours < 0.999


def test_ssim_plane_saturated_16bit(backend):
    """7 x 7, all m against all 0 at 16 bits: one window whose sum of squares, 49 * 65535^2, overflows 32 bits"""
    ops, dev, _ = backend
    a, b = np.full((7, 7), 65535, "<u2"), np.zeros((7, 7), "<u2")
    ref = ssim_plane_ref(a, b, 65535)
    assert 0.0 < ref < 1e-3                                 # S = C1 / (ux^2 + C1) with ux = m
    fmt = _fmt(7, 7, 444, 16)
    pa, pb = (_place(p, dev) for p in _payloads444(a, b))
    ours = float(ops.ssim_plane(pa, pb, fmt, 0).item())
    assert abs(ours - ref) <= SSIM_TOL, (ours, ref)
    assert float(ops.ssim_plane(pa, pb, fmt, 2).item()) == 1.0


@pytest.mark.parametrize("depth", [8, 12, 16])
def test_ssim_plane_unaligned_pointer(backend, depth):
    """30 x 48 takes the 16-byte loads from an aligned payload; one sample further on the same planes take the sample-wide loads"""
    ops, dev, _ = backend
    H, W = 30, 48
    a, b, ref = _plane_pair("random", depth, H, W)
    fmt = _fmt(H, W, 444, depth)
    ya, yb = _payloads444(a, b)
    es = 2 if depth > 8 else 1
    aligned = [ops.ssim_plane(_place(ya, dev), _place(yb, dev), fmt, p).item() for p in range(3)]
    shifted = [ops.ssim_plane(_place(ya, dev, es), _place(yb, dev, es), fmt, p).item() for p in range(3)]
    assert aligned == shifted and abs(aligned[0] - ref) <= SSIM_TOL and aligned[2] == 1.0


def test_ssim_plane_chroma_planes(backend):
    """planes 1 and 2 of a 4:2:0 payload have the chroma shape (19 x 27 here: odd in both axes) and start inside the payload"""
    ops, dev, _ = backend
    fmt = _fmt(38, 54, 420, 10)
    rng = np.random.default_rng(11)
    pa, pb = _samples(rng, fmt.frame_bytes // 2, 10), _samples(rng, fmt.frame_bytes // 2, 10)
    da, db = _place(pa, dev), _place(pb, dev)
    for p, (x, y) in enumerate(zip(fmt.planes(pa.view(np.uint8)), fmt.planes(pb.view(np.uint8)))):
        assert x.shape == ((38, 54) if p == 0 else (19, 27))
        ours = float(ops.ssim_plane(da, db, fmt, p).item())
        assert abs(ours - ssim_plane_ref(x, y, 1023)) <= SSIM_TOL, p


def test_ssim_plane_agrees_with_ssim_u8_on_a_grey_frame(backend):
    ops, dev, _ = backend
    H, W = 37, 53
    a, b, ref = _plane_pair("random", 8, H, W)
    fa, fb = (torch.from_numpy(np.repeat((p.astype(np.float32) / np.float32(255))[None, None], 3, axis=1)).contiguous().to(dev) for p in (a, b))
    rgb = ops.ssim_u8(fa, fb)
    pa, pb = (_place(p, dev) for p in _payloads444(a, b))
    ours = float(ops.ssim_plane(pa, pb, _fmt(H, W, 444, 8), 0).item())
    assert abs(ours - rgb) <= SSIM_TOL and abs(rgb - ref) <= SSIM_TOL, (ours, rgb, ref)
    assert abs(float(ops.ssim_u8_dev(fa, fb).item()) - rgb) == 0.0 and int(ops.sqdiff_u8(fa, fb).item()) == 3 * int(
        ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())


def test_ssim_plane_deterministic_and_out(backend):
    ops, dev, _ = backend
    a, b, _ = _plane_pair("random", 16, 37, 53)
    fmt = _fmt(37, 53, 444, 16)
    pa, pb = (_place(p, dev) for p in _payloads444(a, b))
    first = ops.ssim_plane(pa, pb, fmt, 0).item()
    row = torch.full((3,), -1.0, dtype=torch.float64, device=dev)
    ops.ssim_plane(pa, pb, fmt, 0, out=row[1:2])
    assert row.tolist() == [-1.0, first, -1.0]


def test_ssim_plane_refuses_small_planes_and_bad_arguments(backend):
    ops, dev, _ = backend
    for H, W in ((6, 32), (32, 6)):
        fmt = _fmt(H, W, 444, 8)
        p = torch.zeros(fmt.frame_bytes, dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match="1001"):
            ops.ssim_plane(p, p, fmt, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    part, out = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    ops.lib.call("zt_ssim_plane", buf, buf, 16, 16, 8, part, 4, out, None)
    for args in ((None, buf, 16, 16, 8, part, 4, out), (buf, None, 16, 16, 8, part, 4, out), (buf, buf, 16, 16, 11, part, 4, out),
                 (buf, buf, 16, 16, 8, None, 4, out), (buf, buf, 16, 16, 8, part, 4, None), (buf, buf, 16, 16, 8, part, 0, out),
                 (buf[1:], buf, 16, 16, 10, part, 4, out), (buf, buf, 40, 16, 16, part, 2, out)):
        with pytest.raises(RuntimeError, match="1001"):
            ops.lib.call("zt_ssim_plane", *args, None)
