"""Raw video in and out: the colour-conversion kernels of zt_yuv.hip against the integer definition restated here in
numpy int64 and against an independent float64 statement of BT.601 / BT.709, the Y4M container on the host, InferStep(yuv=) and
predict.py --y4m_in / --y4m_out.  What is pinned is this definition; agreement with libswscale's rounding is not."""
import argparse
import importlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT

KRKB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
COMBOS = [(ss, sit, m, full) for ss, sit in ((420, 0), (420, 1), (422, 0), (422, 1), (444, 0)) for m in ("bt601", "bt709") for full in (0, 1)]
assert len(COMBOS) == 20
# H x W: every neighbour clamped; tails in both axes; one row pair across a 256-thread block of pixel pairs; the vector path
# (W % 8 == 0) with more than 256 patches of 2 x 8
SIZES = [(2, 2), (38, 52), (6, 258), (24, 200)]


def _y4m():
    return importlib.import_module("zero-tig_amd.y4m")


def _fmt(H, W, combo):
    ss, sit, m, full = combo
    return _y4m().YuvFormat(W, H, ss, sit, m, full)


def _cid(c):
    return "%d-%s-%s-%s" % (c[0], "left" if c[1] else "centre", c[2], "full" if c[3] else "limited")


# ------------------------------------------------------------------------------------- the definition, restated (numpy int64)
def _consts(matrix, full):
    kr, kb = KRKB[matrix]
    kg = 1.0 - kr - kb
    cy, cs, yo = (1.0, 1.0, 0) if full else (255.0 / 219.0, 255.0 / 224.0, 16)
    return kr, kg, kb, cy, cs, yo


def _r14(v):
    return int(round(v * 2 ** 14))


def _up16(C, H, W, ss, sit):
    """chroma plane [Hc][Wc] -> int64 [H][W], 16x"""
    C = C.astype(np.int64)
    if ss == 444:
        return 16 * C
    Hc, Wc = C.shape
    x = np.arange(W)
    c = x >> 1
    if sit == 0:
        nb = np.clip(np.where(x % 2 == 0, c - 1, c + 1), 0, Wc - 1)
        h = 3 * C[:, c] + C[:, nb]
    else:
        h = np.where(x % 2 == 0, 4 * C[:, c], 2 * C[:, c] + 2 * C[:, np.minimum(c + 1, Wc - 1)])
    if ss == 422:
        return 4 * h
    y = np.arange(H)
    r = y >> 1
    nb = np.clip(np.where(y % 2 == 0, r - 1, r + 1), 0, Hc - 1)
    return 3 * h[r] + h[nb]


def ref_decode(payload, fmt):
    """payload -> uint8 [H][W][3] by the integer definition"""
    kr, kg, kb, cy, cs, yo = _consts(fmt.matrix, fmt.full)
    CY, CRV, CGU, CGV, CBU = _r14(cy), _r14(cs * 2 * (1 - kr)), _r14(cs * 2 * kb * (1 - kb) / kg), _r14(cs * 2 * kr * (1 - kr) / kg), \
        _r14(cs * 2 * (1 - kb))
    Y, U, V = fmt.planes(payload)
    y = 16 * CY * (Y.astype(np.int64) - yo)
    u = _up16(U, fmt.H, fmt.W, fmt.ss, fmt.siting) - 2048
    v = _up16(V, fmt.H, fmt.W, fmt.ss, fmt.siting) - 2048
    acc = np.stack([y + CRV * v, y - CGU * u - CGV * v, y + CBU * u], axis=-1)
    assert np.abs(acc).max() < 2 ** 31 - 2 ** 17
    return np.clip((acc + 2 ** 17) >> 18, 0, 255).astype(np.uint8)


def _foot(P, ss, sit):
    """integer plane [H][W] -> (footprint sums [Hc][Wc], shift)"""
    P = P.astype(np.int64)
    if ss == 444:
        return P, 0
    H, W = P.shape
    if sit == 0:
        s, sh = P[:, 0::2] + P[:, 1::2], 1
    else:
        xl = np.maximum(np.arange(0, W, 2) - 1, 0)
        s, sh = P[:, xl] + 2 * P[:, 0::2] + P[:, 1::2], 2
    if ss == 420:
        s, sh = s[0::2] + s[1::2], sh + 1
    return s, sh


def quant(x):
    """predict.py save_images, as test_output_side_quantise_and_psnr states it: fp32 [3][H][W] -> uint8 [H][W][3]"""
    return np.transpose(np.clip(x.astype(np.float32) * np.float32(255.0), 0, 255).astype(np.uint8), (1, 2, 0))


def ref_encode(rgb, fmt):
    """uint8 [H][W][3] -> payload by the integer definition"""
    kr, kg, kb, cy, cs, yo = _consts(fmt.matrix, fmt.full)
    R, G, B = (rgb[..., i].astype(np.int64) for i in range(3))
    CYR, CYB = _r14(kr / cy), _r14(kb / cy)
    CYG = _r14(1.0 / cy) - CYR - CYB
    Y = yo + ((CYR * R + CYG * G + CYB * B + 2 ** 13) >> 14)
    (Rs, sh), (Gs, _), (Bs, _) = (_foot(p, fmt.ss, fmt.siting) for p in (R, G, B))
    CUR, CUB = _r14(-kr / (2 * (1 - kb)) / cs), _r14(0.5 / cs)
    CVR, CVB = _r14(0.5 / cs), _r14(-kb / (2 * (1 - kr)) / cs)
    U = 128 + ((CUR * Rs - (CUR + CUB) * Gs + CUB * Bs + 2 ** (13 + sh)) >> (14 + sh))
    V = 128 + ((CVR * Rs - (CVR + CVB) * Gs + CVB * Bs + 2 ** (13 + sh)) >> (14 + sh))
    return np.concatenate([np.clip(p, 0, 255).astype(np.uint8).reshape(-1) for p in (Y, U, V)])


# ------------------------------------------------------------------------- the independent statement (float64, no 2^14 anywhere)
def _upf(C, H, W, ss, sit):
    """bilinear chroma upsampling in float64: sample c of a subsampled axis sits at luma position 2c + 0.5 (centre) or 2c (left)"""
    C = C.astype(np.float64)
    if ss == 444:
        return C

    def axis(A, n_out, pos0):                               # along axis 1
        n = A.shape[1]
        t = (np.arange(n_out) - pos0) / 2.0                 # position in chroma samples
        i0 = np.floor(t).astype(np.int64)
        f = t - i0
        return A[:, np.clip(i0, 0, n - 1)] * (1 - f) + A[:, np.clip(i0 + 1, 0, n - 1)] * f
    h = axis(C, W, 0.5 if sit == 0 else 0.0)
    return h if ss == 422 else axis(h.T, H, 0.5).T


def float_decode(payload, fmt):
    kr, kg, kb, cy, cs, yo = _consts(fmt.matrix, fmt.full)
    Y, U, V = fmt.planes(payload)
    y = (Y.astype(np.float64) - yo) * cy
    pb = (_upf(U, fmt.H, fmt.W, fmt.ss, fmt.siting) - 128.0) * cs       # scaled to B' - Y' = 2 (1 - Kb) Pb
    pr = (_upf(V, fmt.H, fmt.W, fmt.ss, fmt.siting) - 128.0) * cs
    r = y + 2 * (1 - kr) * pr
    b = y + 2 * (1 - kb) * pb
    g = (y - kr * r - kb * b) / kg
    return np.stack([r, g, b], axis=-1)


def float_encode(rgb, fmt):
    """-> float planes (Y, U, V) before rounding"""
    kr, kg, kb, cy, cs, yo = _consts(fmt.matrix, fmt.full)
    R, G, B = (rgb[..., i].astype(np.float64) for i in range(3))
    Y = yo + (kr * R + kg * G + kb * B) / cy

    def mean(P):
        """the colour the chroma sample stands for, written on its own (not through `_foot`): the mean of the two columns a
        centred sample lies between, or the (1/4, 1/2, 1/4) triangle around the column a left-sited sample lies on, whose left
        arm at the plane's edge falls back on column 0; for 4:2:0 the mean of the two rows the sample lies between"""
        P = P.astype(np.float64)
        if fmt.ss == 444:
            return P
        out = np.empty((P.shape[0], P.shape[1] // 2))
        for c in range(out.shape[1]):
            if fmt.siting == 0:
                out[:, c] = 0.5 * P[:, 2 * c] + 0.5 * P[:, 2 * c + 1]
            else:
                out[:, c] = 0.25 * P[:, 2 * c - 1 if c else 0] + 0.5 * P[:, 2 * c] + 0.25 * P[:, 2 * c + 1]
        if fmt.ss == 420:
            out = np.stack([0.5 * (out[2 * r] + out[2 * r + 1]) for r in range(out.shape[0] // 2)])
        return out
    Rm, Gm, Bm = mean(rgb[..., 0]), mean(rgb[..., 1]), mean(rgb[..., 2])
    Ym = kr * Rm + kg * Gm + kb * Bm
    return Y, 128.0 + (Bm - Ym) / (2 * (1 - kb)) / cs, 128.0 + (Rm - Ym) / (2 * (1 - kr)) / cs


# ------------------------------------------------------------------------------------------------------------------ inputs
_CASES = {}


def case(H, W, combo):
    """(fmt, random payload over all 256 codes, fp32 planes in [-0.1, 1.1]) -- made once, never modified"""
    key = (H, W, combo)
    if key not in _CASES:
        fmt = _fmt(H, W, combo)
        rng = np.random.default_rng(1000 * H + W + 7 * COMBOS.index(combo))
        payload = rng.integers(0, 256, fmt.frame_bytes, dtype=np.uint8)
        x = rng.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
        payload.setflags(write=False), x.setflags(write=False)
        _CASES[key] = (fmt, payload, x)
    return _CASES[key]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------ 1. decode
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_decode_definition(backend, combo):
    ops, dev, _ = backend
    for H, W in SIZES:
        fmt, payload, _ = case(H, W, combo)
        got = ops.yuv_to_rgb_u8(_dev(payload, dev), fmt).cpu().numpy()
        assert got.shape == (H, W, 3) and got.dtype == np.uint8
        assert np.array_equal(got, ref_decode(payload, fmt)), (H, W)
        err = np.abs(got.astype(np.float64) - np.clip(float_decode(payload, fmt), 0, 255)).max()
        print("decode %s %dx%d max |u8 - float| = %.4f" % (_cid(combo), H, W, err))
        assert err <= 0.51, (H, W, err)


# ------------------------------------------------------------------------------------------------------ 2. fused decode
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_fused_decode(backend, combo):
    ops, dev, _ = backend
    table = importlib.import_module("zero-tig_amd.ingest").to_tensor_lut()
    for H, W in SIZES:
        assert H * W % 4 == 0
        fmt, payload, _ = case(H, W, combo)
        p = _dev(payload, dev)
        fused = ops.yuv_to_planar_f32(p, fmt)
        u8 = ops.yuv_to_rgb_u8(p, fmt)
        assert torch.equal(fused, ops.ingest_u8(u8, size=None)), (H, W)
        if (H, W) in ((2, 2), (6, 258)):
            assert np.array_equal(fused.cpu().numpy()[0], np.transpose(table[u8.cpu().numpy()], (2, 0, 1))), (H, W)


# ------------------------------------------------------------------------------------------------------------ 3. encode
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_encode_definition(backend, combo):
    ops, dev, _ = backend
    for H, W in SIZES:
        fmt, _, x = case(H, W, combo)
        xd = _dev(x, dev)[None]
        got = ops.rgb_f32_to_yuv(xd, fmt).cpu().numpy()
        rgb = quant(x)
        assert H * W < 100 or (rgb.min() == 0 and rgb.max() == 255)      # clipping on both sides is exercised
        assert got.shape == (fmt.frame_bytes,) and np.array_equal(got, ref_encode(rgb, fmt)), (H, W)
        q = ops.quantize_u8(xd, 0).cpu().numpy()                         # the library's own quantisation
        assert np.array_equal(q, rgb) and np.array_equal(got, ref_encode(q, fmt)), (H, W)
        err = max(np.abs(g.astype(np.float64) - np.clip(f, 0, 255)).max() for g, f in zip(fmt.planes(got), float_encode(rgb, fmt)))
        print("encode %s %dx%d max |u8 - float| = %.4f" % (_cid(combo), H, W, err))
        assert err <= 0.51, (H, W, err)


def test_argument_errors(backend):
    ops, dev, _ = backend
    Y = _y4m().YuvFormat
    p = torch.zeros(64, dtype=torch.uint8, device=dev)
    for bad in (Y(5, 4, 420, 0, "bt709", 0), Y(4, 5, 420, 1, "bt709", 0), Y(5, 4, 422, 1, "bt709", 0), Y(4, 4, 444, 1, "bt709", 0),
                Y(4, 4, 411, 0, "bt709", 0)):
        with pytest.raises(ValueError):
            ops.yuv_to_rgb_u8(p, bad)
    coef = Y(4, 4, 420, 0, "bt709", 0).decode_coef()
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    for H, W, ss, sit in ((4, 5, 420, 0), (5, 4, 420, 0), (4, 5, 422, 0), (4, 4, 444, 1), (4, 4, 411, 0), (0, 4, 444, 0)):
        with pytest.raises(RuntimeError, match="1001"):                 # the library's own argument check
            ops.lib.call("zt_yuv_to_rgb_u8", p, out, H, W, ss, sit, coef, None)


# -------------------------------------------------------------------------------------------------------- 4. properties
# flat colours: the corners of the RGB cube, mid grey, and colours inside the cube
FLAT = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)] + [(128, 128, 128), (200, 120, 40), (30, 90, 160), (90, 200, 60),
                                                                            (250, 240, 20), (16, 16, 32), (180, 60, 200)]


def _levels(rgb_hwc):
    """uint8 [H][W][3] -> fp32 [1][3][H][W] whose truncating quantisation gives these levels back"""
    return torch.from_numpy(np.ascontiguousarray((np.transpose(rgb_hwc, (2, 0, 1)).astype(np.float32) + np.float32(0.5)) / np.float32(255.0))[None])


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_properties(backend, combo):
    ops, dev, _ = backend
    kr, kg, kb, cy, cs, yo = _consts(combo[2], combo[3])
    # grey ramp: no chroma at all, closed-form luma
    H, W = 4, 256
    fmt = _fmt(H, W, combo)
    g = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (H, W, 3))
    Y, U, V = fmt.planes(ops.rgb_f32_to_yuv(_levels(g).to(dev), fmt).cpu().numpy())
    assert (U == 128).all() and (V == 128).all()
    assert np.array_equal(Y, np.broadcast_to(yo + ((_r14(1.0 / cy) * np.arange(256, dtype=np.int64) + 2 ** 13) >> 14), (H, W)))
    # flat colours survive the round trip within 1
    fmt = _fmt(4, 8, combo)
    worst = 0
    for colour in FLAT:
        img = np.broadcast_to(np.array(colour, np.uint8), (4, 8, 3))
        back = ops.yuv_to_rgb_u8(ops.rgb_f32_to_yuv(_levels(img).to(dev), fmt), fmt).cpu().numpy()
        worst = max(worst, int(np.abs(back.astype(np.int64) - img).max()))
    print("flat round trip %s: max %d" % (_cid(combo), worst))
    assert worst <= 1, worst
    # a smooth ramp survives the round trip (chroma subsampled and interpolated back) within 3.  Smooth = at most one level per
    # pixel along either axis in every channel: at the plane's edges the clamped filters place chroma up to one pixel off, an error
    # of at most (slope of the channel - slope of luma) x 1 pixel <= about 1.3 levels on top of the two roundings (at most 1.64
    # for blue: 0.5 x 255/219 from Y plus 0.5 x 2 (1 - Kb) 255/224 from U), so 3 holds for such a ramp and not for a steeper one
    H, W = 32, 48
    fmt = _fmt(H, W, combo)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([40 + xx, 60 + yy, 220 - xx - yy], axis=-1).astype(np.uint8)
    back = ops.yuv_to_rgb_u8(ops.rgb_f32_to_yuv(_levels(ramp).to(dev), fmt), fmt).cpu().numpy()
    worst = int(np.abs(back.astype(np.int64) - ramp).max())
    print("ramp round trip %s: max %d" % (_cid(combo), worst))
    assert worst <= 3, worst


# ---------------------------------------------------------------------------------------------------- 5. host (no kernels)
def test_header_variants():
    y = _y4m()
    h = y.parse_header(b"YUV4MPEG2 W1920 H1080 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED\n")
    assert h == y.Header(1920, 1080, "30000:1001", "p", "1:1", "420mpeg2", "LIMITED") and not h.full
    assert h.format() == y.YuvFormat(1920, 1080, 420, 1, "bt709", 0) and h.format("bt601").matrix == "bt601"
    h = y.parse_header(b"YUV4MPEG2 H6 W10")                               # no C: C420; order is free; no newline
    assert (h.W, h.H, h.ctag, h.fps, h.interlace, h.color_range) == (10, 6, "420", None, None, None)
    assert h.format().ss == 420 and h.format().siting == 1 and h.format().full == 0
    h = y.parse_header(b"YUV4MPEG2 XCOLORRANGE=FULL C444 F25:1 H5 W7 I?\n")
    assert h.full == 1 and h.format() == y.YuvFormat(7, 5, 444, 0, "bt709", 1) and h.format().frame_bytes == 105
    assert y.parse_header(b"YUV4MPEG2 W4 H4 C420jpeg\n").format().siting == 0
    assert y.parse_header(b"YUV4MPEG2 W4 H4 C420paldv\n").format().siting == 1
    assert y.parse_header(b"YUV4MPEG2 W4 H3 C422\n").format().frame_bytes == 24
    for hd in (h, y.Header(10, 6, None, None, None, "420", None), y.Header(1920, 1080, "30000:1001", "p", "1:1", "420mpeg2", "LIMITED")):
        assert y.parse_header(hd.to_bytes()) == hd


@pytest.mark.parametrize("line,field", [
    (b"YUV4MPEG2 W4 H4 It C420\n", "It"), (b"YUV4MPEG2 W4 H4 Im\n", "Im"), (b"YUV4MPEG2 W4 H4 C420p10\n", "C420p10"),
    (b"YUV4MPEG2 W4 H4 C422p12\n", "C422p12"), (b"YUV4MPEG2 W4 H4 C444p16\n", "C444p16"), (b"YUV4MPEG2 W4 H4 Cmono\n", "Cmono"),
    (b"YUV4MPEG2 W4 H4 C444alpha\n", "C444alpha"), (b"YUV4MPEG2 W5 H4 C420\n", "W5"), (b"YUV4MPEG2 W4 H5\n", "H5"),
    (b"YUV4MPEG2 W5 H4 C422\n", "W5"), (b"YUV4MPEG2 H4\n", "W"), (b"YUV4MPEG2 W4 H4 F30\n", "F30"),
    (b"YUV4MPEG2 W4 H4 XCOLORRANGE=WIDE\n", "XCOLORRANGE"), (b"YUV4MPEG W4 H4\n", "YUV4MPEG2")])
def test_header_rejections_name_the_field(line, field):
    with pytest.raises(ValueError, match=field):
        _y4m().parse_header(line)


def _clip(tmp_path, ctag, n=7, W=10, H=6, full=None):
    y = _y4m()
    head = y.Header(W, H, "25:1", "p", None, ctag, full)
    rng = np.random.default_rng(5)
    payloads = [rng.integers(0, 256, head.format().frame_bytes, dtype=np.uint8) for _ in range(n)]
    path = tmp_path / ("clip_%s.y4m" % ctag)
    y.write_file(str(path), head, payloads)
    return path, head, payloads


@pytest.mark.parametrize("ctag", ["420mpeg2", "422", "444"])
def test_writer_reader_round_trip(tmp_path, ctag):
    y = _y4m()
    _, head, payloads = _clip(tmp_path, ctag, full="FULL" if ctag == "444" else None)
    path = tmp_path / "w.y4m"
    w = y.Y4MWriter(str(path), head, slots=2)
    for i, p in enumerate(payloads):
        w.submit(p if i % 2 else torch.from_numpy(p))
    w.close()
    assert w.frames == 7 and path.stat().st_size == w.bytes + len(head.to_bytes())
    r = y.Y4MReader(str(path), slots=2)
    assert r.header == head
    got = [f.numpy().copy() for f in r]
    assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got, payloads))
    with pytest.raises(StopIteration):
        next(r)


def test_reader_truncated_last_frame_raises(tmp_path):
    y = _y4m()
    path, head, payloads = _clip(tmp_path, "420mpeg2")
    data = path.read_bytes()
    (tmp_path / "cut.y4m").write_bytes(data[:-5])
    r = y.Y4MReader(str(tmp_path / "cut.y4m"))
    got = []
    with pytest.raises(ValueError, match="truncated"):
        for f in r:
            got.append(f.numpy().copy())
    assert len(got) == 6 and np.array_equal(got[5], payloads[5])
    (tmp_path / "nohead.y4m").write_bytes(b"YUV4MPEG2 W10 H6")
    with pytest.raises(ValueError, match="header"):
        y.Y4MReader(str(tmp_path / "nohead.y4m"))


def test_reader_close_leaves_no_thread(tmp_path):
    """at the end of the stream, and when the consumer stops early (ring and queue full), close() returns with the reader's
    thread gone: a thread left running into the interpreter's shutdown can abort the process"""
    y = _y4m()
    path, head, payloads = _clip(tmp_path, "444")
    r = y.Y4MReader(str(path), slots=2)
    assert len(list(r)) == 7 and not r._thread.is_alive()
    r = y.Y4MReader(str(path), slots=2)
    assert np.array_equal(next(r).numpy(), payloads[0])
    r.close()
    assert not r._thread.is_alive()
    with pytest.raises(StopIteration):
        next(r)


def test_reader_from_a_pipe(tmp_path):
    path, head, payloads = _clip(tmp_path, "422")
    code = ("import importlib, sys, hashlib; sys.path.insert(0, %r); y = importlib.import_module('zero-tig_amd.y4m'); "
            "r = y.Y4MReader('-'); print(r.header.to_bytes().decode().strip()); "
            "[print(hashlib.sha1(f.numpy().tobytes()).hexdigest()) for f in r]" % ROOT)
    cat = subprocess.Popen(["cat", str(path)], stdout=subprocess.PIPE)
    out = subprocess.run([sys.executable, "-c", code], stdin=cat.stdout, capture_output=True, text=True, timeout=120)
    cat.stdout.close()
    assert cat.wait(60) == 0 and out.returncode == 0, out.stderr[-2000:]
    import hashlib
    lines = out.stdout.split("\n")[:-1]
    assert lines[0] == head.to_bytes().decode().strip()
    assert lines[1:] == [hashlib.sha1(p.tobytes()).hexdigest() for p in payloads]


def test_y4m_writer_bounded_queue_blocks(tmp_path):
    y = _y4m()
    gate, opened = threading.Event(), threading.Event()

    def slow_open(path, mode):
        opened.set()
        assert gate.wait(60)
        return open(path, mode)
    head = y.Header(4, 2, None, None, None, "444", None)
    frame = np.arange(24, dtype=np.uint8)
    w = y.Y4MWriter(str(tmp_path / "o.y4m"), head, slots=2, open_fn=slow_open)
    w.submit(frame)
    assert opened.wait(60)                                  # the thread holds frame 0; the queue takes two more
    w.submit(frame)
    w.submit(frame)
    t = threading.Thread(target=w.submit, args=(frame,), daemon=True)
    t.start()
    t.join(0.5)
    assert t.is_alive(), "a full queue must block the producer"
    gate.set()
    t.join(60)
    assert not t.is_alive()
    w.close()
    assert w.frames == 4 and w.wait_writer >= 0.4
    assert (tmp_path / "o.y4m").read_bytes() == head.to_bytes() + (b"FRAME\n" + frame.tobytes()) * 4


def test_y4m_writer_failure_surfaces(tmp_path):
    y = _y4m()
    head = y.Header(4, 2, None, None, None, "444", None)
    frame = np.zeros(24, np.uint8)

    def bad_open(path, mode):
        raise OSError("disk full: " + path)
    w = y.Y4MWriter(str(tmp_path / "o.y4m"), head, slots=2, open_fn=bad_open)
    for _ in range(5):                                      # later frames are released, not written: nothing hangs
        try:
            w.submit(frame)
        except OSError:
            break
    with pytest.raises(OSError, match="disk full"):
        w.close()
    assert w.frames == 0
    # a sink that goes away mid-stream (the reader of a pipe exits): submit() raises once the thread has met the error
    rd, wr = os.pipe()
    os.close(rd)
    w = y.Y4MWriter("-", head, slots=2, fh=os.fdopen(wr, "wb", buffering=0))
    raised = None
    for _ in range(200):
        try:
            w.submit(frame)
        except BrokenPipeError as e:
            raised = e
            break
    assert raised is not None, "submit() must not swallow a broken pipe"
    with pytest.raises(BrokenPipeError):
        w.close()


# -------------------------------------------------------------------------------------------------------- 6. InferStep
def _net(ops, dev, synth, precision, seed=1):
    net_mod = importlib.import_module("zero-tig_amd.network")
    net = net_mod.Finetunemodel(argparse.Namespace(dataset="RLV", of_scale=1), ops=ops, precision=precision)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(seed).items()})
    return net.to(dev).eval()


def _synth_payloads(synth, fmt, n):
    out = []
    for t in range(n):
        a = np.asarray(synth.lowlight_frame(t, fmt.H, fmt.W), dtype=np.float32)
        rgb = (np.transpose(a[0] if a.ndim == 4 else a, (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
        out.append(ref_encode(rgb, fmt))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,ctag,full,precision", [(128, 160, "420mpeg2", None, "bf16"), (128, 160, "420mpeg2", None, "fp32"),
                                                     (128, 160, "444", "FULL", "bf16"), (48, 64, "444", "FULL", "bf16")])
def test_inferstep_yuv(hip_ops, synth, H, W, ctag, full, precision):
    """5 frames through InferStep(yuv=) with and without the graph, and through an InferStep without yuv that is fed the RGB frame
    `Ops.yuv_to_rgb_u8` makes: H2, H3, both uint8 images and both output payloads agree bit for bit, the payloads are the encode of
    H2 / H3, and the graph is captured once and engages from the third frame.  of_scale 1, as in test_infer.py at this size.
    48 x 64 is below what RAFT's four-level correlation pyramid takes (H / 8 >= 8), so there every frame starts a sequence, as in
    test_inferstep_folded_batchnorm, and nothing is captured."""
    ops, dev = hip_ops
    steady = H >= 64
    infer = importlib.import_module("zero-tig_amd.infer")
    fmt = _y4m().Header(W, H, None, None, None, ctag, full).format("bt709")
    graph = infer.InferStep(_net(ops, dev, synth, precision), use_graph=True, ingest_size=None, yuv=fmt)
    eager = infer.InferStep(_net(ops, dev, synth, precision), use_graph=False, ingest_size=None, yuv=fmt)
    plain = infer.InferStep(_net(ops, dev, synth, precision), use_graph=False, ingest_size=None)
    assert graph.yuv_format == fmt
    for t, payload in enumerate(_synth_payloads(synth, fmt, 5)):
        pinned = torch.from_numpy(payload).pin_memory()
        new = t == 0 or not steady
        g = graph(pinned, is_new_seq=new)
        assert (graph.graph is not None) == (steady and t >= 2)
        e = eager(torch.from_numpy(payload).to(dev), is_new_seq=new)
        p = plain(ops.yuv_to_rgb_u8(torch.from_numpy(payload).to(dev), fmt), is_new_seq=new)
        for i in (0, 1):
            assert torch.equal(g[i], e[i]) and torch.equal(g[i], p[i]), (t, i)
            assert torch.equal(graph.yuv[i], eager.yuv[i]), (t, i)
            assert torch.equal(graph.yuv[i], ops.rgb_f32_to_yuv(graph.out[i], fmt)), (t, i)
            assert torch.equal(graph.u8[i], plain.u8[i]), (t, i)
    assert graph.n_captures == (1 if steady else 0)


# ---------------------------------------------------------------------------------------------------------- 7. scripts
def _run(script, *args, ok=True, stdin=None, binary=False):
    r = subprocess.run([sys.executable, script] + [str(a) for a in args], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=not binary, timeout=600, stdin=stdin)
    if ok:
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r


def _frames_of(path):
    y = _y4m()
    r = y.Y4MReader(str(path), pin=False)
    return r.header, [f.numpy().copy() for f in r]


@pytest.mark.gpu
def test_scripts_y4m(tmp_path, synth):
    y = _y4m()
    n, H, W = 4, 270, 480
    head = y.Header(W, H, "30000:1001", "p", None, "420mpeg2", "LIMITED")
    fmt = head.format("bt709")
    payloads = _synth_payloads(synth, fmt, n)
    src = tmp_path / "clip.y4m"
    y.write_file(str(src), head, payloads)
    weights = tmp_path / "weights.pt"
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, str(weights))
    # the same four frames as PNGs of their decoded RGB, in the RLV layout
    d = tmp_path / "data" / "RLV" / "input" / "S01" / "low_light_10"
    d.mkdir(parents=True)
    for t, p in enumerate(payloads):
        Image.fromarray(ref_decode(p, fmt)).save(str(d / ("%05d.png" % (t + 1))))
    (tmp_path / "data" / "RLV" / "test_list.txt").write_text("S01\n")
    _run("predict.py", "--dataset", "RLV", "--lowlight_images_path", tmp_path / "data" / "RLV", "--model_pretrain", weights, "--save",
         tmp_path / "png", "--graph", "1", "--device_png", "0")
    common = ("--model_pretrain", weights, "--graph", "1")
    _run("predict.py", *common, "--save", tmp_path / "big", "--y4m_in", src, "--y4m_resize", "1")
    big = fmt.resized(1920, 1080)
    for kind in ("enhance", "denoise"):
        h, frames = _frames_of(tmp_path / "big" / ("clip_%s.y4m" % kind))
        assert h == head.resized(1920, 1080) and len(frames) == n, (kind, h, len(frames))
        for t, f in enumerate(frames):
            png = np.asarray(Image.open(str(tmp_path / "png" / "S01" / "low_light_10" / ("%05d_%s.png" % (t + 1, kind)))))
            assert png.shape == (1080, 1920, 3) and np.array_equal(f, ref_encode(png, big)), (kind, t)
    # native size: RAFT's correlation pyramid needs (H / of_scale) / 8 >= 8, which 270 rows give at --of_scale 1, not at the default 3
    _run("predict.py", *common, "--of_scale", "1", "--save", tmp_path / "small", "--y4m_in", src)
    for kind in ("enhance", "denoise"):
        h, frames = _frames_of(tmp_path / "small" / ("clip_%s.y4m" % kind))
        assert h == head and len(frames) == n, (kind, h, len(frames))
    with open(str(src), "rb") as fh:                         # file -> pipe -> predict.py -> pipe
        cat = subprocess.Popen(["cat"], stdin=fh, stdout=subprocess.PIPE)
        r = _run("predict.py", *common, "--of_scale", "1", "--y4m_in", "-", "--y4m_out", "-", stdin=cat.stdout, binary=True)
        cat.stdout.close()
        assert cat.wait(60) == 0
    assert r.stdout == (tmp_path / "small" / "clip_enhance.y4m").read_bytes()
    # --y4m_out PATH: the enhance stream alone, at that path; no denoise stream and nothing under --save
    _run("predict.py", *common, "--of_scale", "1", "--save", tmp_path / "unused", "--y4m_in", src, "--y4m_out", tmp_path / "only.y4m")
    assert (tmp_path / "only.y4m").read_bytes() == r.stdout and not (tmp_path / "unused").exists()
    for extra, word in ((("--graph", "0"), "--graph 1"), (("--graph", "1", "--device_png", "1"), "--device_png")):
        r = _run("predict.py", "--model_pretrain", weights, "--save", tmp_path / "no", "--y4m_in", src, *extra, ok=False)
        assert r.returncode != 0 and word in r.stderr and "--y4m_in" in r.stderr, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "no").exists()
