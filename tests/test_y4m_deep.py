"""High-bit-depth raw video: the deep kernels of zt_yuv.hip against the integer definition restated here in numpy int64
and against the float64 statement of BT.601 / BT.709 (test_y4m.py's bilinear chroma, no 2^20 anywhere), the scene-cut grid of a
deep plane, the Y4M container with 16-bit samples, InferStep(yuv=, yuv_out_depth=) and predict.py --y4m_out_depth.  What is
pinned is this definition; agreement with libswscale's rounding is not.  The chroma taps (`_up16`, `_upf`, `_foot`) and the flat
colours are test_y4m.py's: they are the same at every depth."""
import importlib

import numpy as np
import pytest
import torch

import test_y4m as t8

COMBOS, SIZES, KRKB = t8.COMBOS, t8.SIZES, t8.KRKB
_cid, _y4m, _dev = t8._cid, t8._y4m, t8._dev
# every size at 10, 12 and 16 bits; 9 and 14 at the size with tails in both axes
DEPTHS = {(2, 2): (10, 12, 16), (38, 52): (9, 10, 12, 14, 16), (6, 258): (10, 12, 16), (24, 200): (10, 12, 16)}
RUNS = [(H, W, B) for (H, W) in SIZES for B in DEPTHS[(H, W)]]


def _fmt(H, W, combo, B):
    ss, sit, m, full = combo
    return _y4m().YuvFormat(W, H, ss, sit, m, full, B)


# ------------------------------------------------------------------------------------- the definition, restated (numpy int64)
def _consts(matrix, full, B):
    kr, kb = KRKB[matrix]
    m, k, mid = 2 ** B - 1, 2 ** (B - 8), 2 ** (B - 1)
    yo, Yr, Cr = (0, m, m) if full else (16 * k, 219 * k, 224 * k)
    return kr, 1.0 - kr - kb, kb, m, mid, yo, Yr, Cr


def _r20(v):
    return int(round(v * 2 ** 20))


def _dec_exact(matrix, full, B):
    """CY, CRV, CGU, CGV, CBU in double precision"""
    kr, kg, kb, m, mid, yo, Yr, Cr = _consts(matrix, full, B)
    cs = 65535.0 / Cr
    return [65535.0 / Yr, cs * 2 * (1 - kr), cs * 2 * kb * (1 - kb) / kg, cs * 2 * kr * (1 - kr) / kg, cs * 2 * (1 - kb)]


def _enc_exact(matrix, full, B):
    """the rows (Y, U, V) x (R, G, B) in double precision"""
    kr, kg, kb, m, mid, yo, Yr, Cr = _consts(matrix, full, B)
    ys, cs = Yr / 65535.0, Cr / 65535.0
    return [[kr * ys, kg * ys, kb * ys],
            [-kr / (2 * (1 - kb)) * cs, -kg / (2 * (1 - kb)) * cs, 0.5 * cs],
            [0.5 * cs, -kg / (2 * (1 - kr)) * cs, -kb / (2 * (1 - kr)) * cs]]


def _enc_table(matrix, full, B):
    """the integer rows: the green entry of Y makes the row sum round(2^20 Yr / 65535), the green entries of U and V make theirs 0"""
    kr, kg, kb, m, mid, yo, Yr, Cr = _consts(matrix, full, B)
    ex = _enc_exact(matrix, full, B)
    CYR, CYB = _r20(ex[0][0]), _r20(ex[0][2])
    CUR, CUB, CVR, CVB = _r20(ex[1][0]), _r20(ex[1][2]), _r20(ex[2][0]), _r20(ex[2][2])
    return [[CYR, _r20(Yr / 65535.0) - CYR - CYB, CYB], [CUR, -(CUR + CUB), CUB], [CVR, -(CVR + CVB), CVB]]


def _planes(payload, fmt):
    """(Y, U, V) of a deep payload as int64, samples above m read as m"""
    p = np.asarray(payload).view("<u2").astype(np.int64)
    hc, wc = fmt.chroma_shape
    n, m = fmt.H * fmt.W, 2 ** fmt.depth - 1
    assert p.size == n + 2 * hc * wc
    return np.minimum(p[:n], m).reshape(fmt.H, fmt.W), np.minimum(p[n:n + hc * wc], m).reshape(hc, wc), np.minimum(p[n + hc * wc:], m).reshape(hc, wc)


def ref_decode16(payload, fmt):
    """payload -> (L16 int64 [H][W][3], float32 [H][W][3]) by the integer definition"""
    kr, kg, kb, m, mid, yo, Yr, Cr = _consts(fmt.matrix, fmt.full, fmt.depth)
    CY, CRV, CGU, CGV, CBU = (_r20(c) for c in _dec_exact(fmt.matrix, fmt.full, fmt.depth))
    Y, U, V = _planes(payload, fmt)
    y = 16 * CY * (Y - yo)
    u = t8._up16(U, fmt.H, fmt.W, fmt.ss, fmt.siting) - 16 * mid
    v = t8._up16(V, fmt.H, fmt.W, fmt.ss, fmt.siting) - 16 * mid
    acc = np.stack([y + CRV * v, y - CGU * u - CGV * v, y + CBU * u], axis=-1)
    assert np.abs(acc).max() < 2 ** 42
    L16 = np.clip((acc + 2 ** 23) >> 24, 0, 65535)
    return L16, L16.astype(np.float32) / np.float32(65535)


def quant16(x):
    """fp32 [3][H][W] -> int64 [H][W][3] 16-bit levels: a float32 multiply, a float32 add, truncation; NaN and x <= 0 give 0, x >= 1
    gives 65535"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * np.float32(65535.0) + np.float32(0.5)
    assert t.dtype == np.float32
    inside = (x > 0) & (x < 1)
    L = np.where(inside, np.where(inside, t, np.float32(0)).astype(np.int64), np.where(x >= 1, 65535, 0))
    return np.transpose(L, (1, 2, 0))


def ref_encode16(L16, fmt):
    """int64 [H][W][3] 16-bit levels -> (payload as uint8, (Y, U, V) int64) by the integer definition"""
    kr, kg, kb, m, mid, yo, Yr, Cr = _consts(fmt.matrix, fmt.full, fmt.depth)
    cy, cu, cv = _enc_table(fmt.matrix, fmt.full, fmt.depth)
    R, G, B = (np.asarray(L16)[..., i].astype(np.int64) for i in range(3))
    Y = yo + ((cy[0] * R + cy[1] * G + cy[2] * B + 2 ** 19) >> 20)
    (Rs, sh), (Gs, _), (Bs, _) = (t8._foot(p, fmt.ss, fmt.siting) for p in (R, G, B))
    U = mid + ((cu[0] * Rs + cu[1] * Gs + cu[2] * Bs + 2 ** (19 + sh)) >> (20 + sh))
    V = mid + ((cv[0] * Rs + cv[1] * Gs + cv[2] * Bs + 2 ** (19 + sh)) >> (20 + sh))
    planes = [np.clip(p, 0, m) for p in (Y, U, V)]
    return np.concatenate([p.astype("<u2").reshape(-1) for p in planes]).view(np.uint8), planes


# ------------------------------------------------------------------------- the independent statement (float64, no 2^20 anywhere)
def float_decode16(payload, fmt):
    """-> float64 [H][W][3] on the 0..65535 scale, unclipped"""
    kr, kg, kb, m, mid, yo, Yr, Cr = _consts(fmt.matrix, fmt.full, fmt.depth)
    Y, U, V = _planes(payload, fmt)
    y = (Y.astype(np.float64) - yo) * (65535.0 / Yr)
    pb = (t8._upf(U, fmt.H, fmt.W, fmt.ss, fmt.siting) - mid) * (65535.0 / Cr)
    pr = (t8._upf(V, fmt.H, fmt.W, fmt.ss, fmt.siting) - mid) * (65535.0 / Cr)
    r = y + 2 * (1 - kr) * pr
    b = y + 2 * (1 - kb) * pb
    g = (y - kr * r - kb * b) / kg
    return np.stack([r, g, b], axis=-1)


def float_encode16(L16, fmt):
    """-> float planes (Y, U, V) in codes of fmt.depth before rounding.  test_y4m.py's float_encode with a full-range 8-bit format
    is the bare statement (Y' = Kr R + Kg G + Kb B, Pb, Pr over the footprint's mean colour, offsets 0 and 128) and takes any
    scale of RGB; the ranges of this depth are applied to it here"""
    kr, kg, kb, m, mid, yo, Yr, Cr = _consts(fmt.matrix, fmt.full, fmt.depth)
    bare = _y4m().YuvFormat(fmt.W, fmt.H, fmt.ss, fmt.siting, fmt.matrix, 1)
    Yp, U, V = t8.float_encode(np.asarray(L16, dtype=np.float64), bare)
    return yo + Yp * (Yr / 65535.0), mid + (U - 128.0) * (Cr / 65535.0), mid + (V - 128.0) * (Cr / 65535.0)


# ------------------------------------------------------------------------------------------------------------------ inputs
_CASES = {}


def case(H, W, combo, B):
    """(fmt, payload, fp32 planes) -- made once, never modified.  The payload is random over 0..m with the codes 0, yo, yo + Yr,
    mid and m planted, and for B < 16 codes above m; the planes are drawn from [-0.1, 1.1] with a black pixel (NaN, -inf, < 0)
    at (0, 0) and a white one (+inf, 1, > 1) at (0, 1)"""
    key = (H, W, combo, B)
    if key not in _CASES:
        fmt = _fmt(H, W, combo, B)
        kr, kg, kb, m, mid, yo, Yr, Cr = _consts(combo[2], combo[3], B)
        rng = np.random.default_rng(100000 * B + 1000 * H + W + 7 * COMBOS.index(combo))
        n = fmt.frame_bytes // 2
        s = rng.integers(0, m + 1, n, dtype=np.uint16)
        special = [0, yo, yo + Yr, mid, m] + ([m + 1, 65535, int(rng.integers(m + 1, 65536))] if B < 16 else [])
        pos = rng.choice(n, min(n // 2, 4 * len(special)), replace=False)
        s[pos] = [special[i % len(special)] for i in range(len(pos))]
        payload = s.astype("<u2").view(np.uint8)
        x = rng.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
        x[:, 0, 0] = (np.nan, -np.inf, -0.05)
        x[:, 0, 1] = (np.inf, 1.0, 1.05)
        payload.setflags(write=False), x.setflags(write=False)
        _CASES[key] = (fmt, payload, x)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------- 1. decode definition
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_decode_definition(backend, combo):
    ops, dev, _ = backend
    for H, W, B in RUNS:
        fmt, payload, _ = case(H, W, combo, B)
        assert np.array_equal(np.asarray(fmt.decode_coef())[1:], [_r20(c) for c in _dec_exact(combo[2], combo[3], B)])
        got = ops.yuv_to_planar_f32(_dev(payload, dev), fmt).cpu().numpy()
        assert got.shape == (1, 3, H, W) and got.dtype == np.float32
        want = np.transpose(ref_decode16(payload, fmt)[1], (2, 0, 1))
        assert np.array_equal(got[0], want), (H, W, B, int((got[0] != want).sum()))


# ------------------------------------------------------------------------------------------------------ 2. decode accuracy
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_decode_accuracy(combo):
    """|L16 - float| <= 0.5 + e: 0.5 is the one rounding; e is what the rounded coefficients can add, per channel the sum over its
    terms of |c / 2^20 - exact| x the largest operand (|Y - yo| <= max(yo, m - yo), |chroma - mid| <= mid; the 16x chroma is
    exact in both statements), plus 1e-6 for the float64 evaluation.  Clipping moves the two values no further apart."""
    worst = 0.0
    for H, W, B in RUNS:
        fmt, payload, _ = case(H, W, combo, B)
        kr, kg, kb, m, mid, yo, Yr, Cr = _consts(combo[2], combo[3], B)
        table = [int(v) for v in fmt.decode_coef()]
        assert table[0] == yo
        dCY, dCRV, dCGU, dCGV, dCBU = (abs(c / 2.0 ** 20 - ex) for c, ex in zip(table[1:], _dec_exact(combo[2], combo[3], B)))
        ymax = max(yo, m - yo)
        e = max(dCY * ymax + dCRV * mid, dCY * ymax + (dCGU + dCGV) * mid, dCY * ymax + dCBU * mid) + 1e-6
        err = np.abs(ref_decode16(payload, fmt)[0] - np.clip(float_decode16(payload, fmt), 0, 65535)).max()
        print("decode16 %s %dx%d B=%d max |L16 - float| = %.4f (bound %.4f)" % (_cid(combo), H, W, B, err, 0.5 + e))
        assert err <= 0.5 + e, (H, W, B, err, e)
        worst = max(worst, err)
    print("decode16 %s worst %.4f" % (_cid(combo), worst))


# ---------------------------------------------------------------------------------------------------- 3. encode definition
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_encode_definition(backend, combo):
    """Bit for bit, the float32 quantisation included.  Both ends of the code range must occur in the result at the three larger
    sizes: 0 and m for full range.  For limited range the definition cannot produce them from any input (levels 0..65535 map onto
    yo..yo + Yr, and chroma onto mid -+ Cr / 2), so there the ends that can occur, yo and yo + Yr, must, and 0 and 65535 among
    the quantised levels."""
    ops, dev, _ = backend
    for H, W, B in RUNS:
        fmt, _, x = case(H, W, combo, B)
        kr, kg, kb, m, mid, yo, Yr, Cr = _consts(combo[2], combo[3], B)
        assert np.array_equal(np.asarray(fmt.encode_coef()), [yo] + sum(_enc_table(combo[2], combo[3], B), []))
        got = ops.rgb_f32_to_yuv(_dev(x, dev)[None], fmt).cpu().numpy()
        L16 = quant16(x)
        want, planes = ref_encode16(L16, fmt)
        assert got.shape == (fmt.frame_bytes,) and got.dtype == np.uint8
        assert np.array_equal(got, want), (H, W, B, int((got != want).sum()))
        if H * W >= 100:
            s = got.view("<u2")
            assert L16.min() == 0 and L16.max() == 65535
            assert ((s == 0).any() and (s == m).any()) if combo[3] else ((s == yo).any() and (s == yo + Yr).any()), (H, W, B)


# ------------------------------------------------------------------------------------------------------ 4. encode accuracy
@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_encode_accuracy(combo):
    """In codes of the output depth, |plane - float| <= 0.5 + e: per plane e is the sum over its three terms of
    |c / 2^20 - exact| x 65535 (a footprint sum over its weight total 2^sh is at most 65535), plus 1e-6 for the float64
    evaluation.  The integer green entries are made by subtraction, so they carry the errors of the other two entries as well;
    the derived bound is about 0.66."""
    worst = 0.0
    for H, W, B in RUNS:
        fmt, _, x = case(H, W, combo, B)
        m = 2 ** B - 1
        table = [int(v) for v in fmt.encode_coef()]
        rows = [table[1:4], table[4:7], table[7:10]]
        es = [sum(abs(c / 2.0 ** 20 - ex) for c, ex in zip(row, exact)) * 65535.0 + 1e-6 for row, exact in zip(rows, _enc_exact(combo[2], combo[3], B))]
        L16 = quant16(x)
        planes = ref_encode16(L16, fmt)[1]
        for name, p, f, e in zip("YUV", planes, float_encode16(L16, fmt), es):
            err = np.abs(p - np.clip(f, 0, m)).max()
            print("encode16 %s %dx%d B=%d %s max |code - float| = %.4f (bound %.4f)" % (_cid(combo), H, W, B, name, err, 0.5 + e))
            assert err <= 0.5 + e, (H, W, B, name, err, e)
            worst = max(worst, err)
    print("encode16 %s worst %.4f" % (_cid(combo), worst))


# ----------------------------------------------------------------------------------------------------------- 5. properties
def _levels16(L):
    """integer levels [H][W][3] -> fp32 [1][3][H][W] whose quantisation gives these levels back"""
    x = (np.transpose(L, (2, 0, 1)).astype(np.float32) / np.float32(65535.0))[None]
    assert np.array_equal(quant16(x[0]), L)
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_grey_and_flat_round_trip(backend, combo):
    ops, dev, _ = backend
    for B in (9, 10, 12, 14, 16):
        kr, kg, kb, m, mid, yo, Yr, Cr = _consts(combo[2], combo[3], B)
        # grey in, no chroma out, closed-form luma: every 255th level and the levels next to the ends of the range
        H, W = 4, 264
        fmt = _fmt(H, W, combo, B)
        lv = np.concatenate([np.arange(0, 65536, 255), [1, 2, 32767, 32768, 65533, 65534]]).astype(np.int64)[:W]
        assert lv.size == W
        g = np.broadcast_to(lv[None, :, None], (H, W, 3))
        got = ops.rgb_f32_to_yuv(_levels16(g).to(dev), fmt).cpu().numpy()
        Y, U, V = (p.astype(np.int64) for p in fmt.planes(got))
        assert (U == mid).all() and (V == mid).all(), B
        assert np.array_equal(Y, np.broadcast_to(yo + ((_r20(Yr / 65535.0) * lv + 2 ** 19) >> 20), (H, W))), B
        # encode, decode, encode of a flat in-gamut colour moves no plane by more than 1 code
        fmt = _fmt(4, 8, combo, B)
        worst = 0
        for colour in t8.FLAT:
            img = np.broadcast_to(np.array(colour, np.int64) * 257, (4, 8, 3))
            first = ops.rgb_f32_to_yuv(_levels16(img).to(dev), fmt)
            second = ops.rgb_f32_to_yuv(ops.yuv_to_planar_f32(first, fmt), fmt)
            d = np.abs(second.cpu().numpy().view("<u2").astype(np.int64) - first.cpu().numpy().view("<u2").astype(np.int64)).max()
            worst = max(worst, int(d))
        print("flat encode-decode-encode %s B=%d: max %d" % (_cid(combo), B, worst))
        assert worst <= 1, (B, worst)


def _truncated(payload, fmt):
    """the 8-bit copy of a deep payload: min(sample, m) >> (B - 8), and its format"""
    s = np.minimum(np.asarray(payload).view("<u2").astype(np.int64), 2 ** fmt.depth - 1) >> (fmt.depth - 8)
    return s.astype(np.uint8), fmt._replace(depth=8)


# 40 x 64 is the grid kernel's 16-byte path (W % 16 == 0) with a row of cells cut by the bottom edge
@pytest.mark.parametrize("H,W", [(38, 52), (24, 200), (40, 64)])
def test_luma_grid_is_the_8bit_grid_of_the_truncated_plane(backend, H, W):
    ops, dev, _ = backend
    for combo in (COMBOS[0], COMBOS[19]):                               # limited (yo 16) and full (yo 0)
        for B in (9, 10, 12, 14, 16):
            fmt = _fmt(H, W, combo, B)
            rng = np.random.default_rng(H + W + B)
            s = rng.integers(0, 2 ** B, fmt.frame_bytes // 2, dtype=np.uint16)
            s[::7] >>= max(B - 12, 0) + 3                               # dark samples, below yo after the shift
            if B < 16:
                s[::11] |= 1 << B                                       # codes above m
            payload = s.astype("<u2").view(np.uint8)
            p8, fmt8 = _truncated(payload, fmt)
            want = ops.luma_grid(_dev(p8, dev), fmt8)
            got = ops.luma_grid(_dev(payload, dev), fmt)
            assert got.dtype == torch.int32 and tuple(got.shape) == ((H + 15) // 16, (W + 15) // 16)
            assert torch.equal(got, want), (combo, B)
            luma = _dev(payload[:2 * H * W], dev)                       # the plane alone, 1-D
            assert torch.equal(ops.luma_grid(luma, fmt), want), (combo, B)
            Y = np.minimum(s[:H * W].astype(np.int64), 2 ** B - 1).reshape(H, W) >> (B - 8)
            cells = np.maximum(Y - (0 if combo[3] else 16), 0)
            cells = np.pad(cells, ((0, -H % 16), (0, -W % 16))).reshape((H + 15) // 16, 16, (W + 15) // 16, 16).sum(axis=(1, 3))
            assert np.array_equal(got.cpu().numpy(), cells), (combo, B)


def test_scenecut_deep_equals_truncated(backend):
    ops, dev, _ = backend
    scenecut = importlib.import_module("zero-tig_amd.scenecut")
    H, W, B = 48, 80, 10
    fmt = _fmt(H, W, COMBOS[4], B)                                      # 420 left bt709 limited
    rng = np.random.default_rng(11)
    base = [rng.integers(64, 400, (H, W)), rng.integers(200, 1000, (H, W))]
    clip = []
    for t in range(6):                                                  # a cut between frames 2 and 3
        Y = base[t // 3] + rng.integers(0, 8, (H, W))
        C = rng.integers(0, 1024, 2 * (H // 2) * (W // 2))
        clip.append(np.concatenate([Y.reshape(-1), C]).astype("<u2").view(np.uint8))
    deep, flat = scenecut.SceneCut(ops, dev, fmt, 0.03), scenecut.SceneCut(ops, dev, fmt._replace(depth=8), 0.03)
    seq = []
    for p in clip:
        p8, _ = _truncated(p, fmt)
        deep.push(_dev(p, dev)), flat.push(_dev(p8, dev))
        a, b = deep.pop(), flat.pop()
        assert a == b, (len(seq), a, b)
        seq.append(a)
    assert [s[0] for s in seq] == [True, False, False, True, False, False], seq


# ------------------------------------------------------------------------------------------------------------ 6. arguments
def test_argument_errors(backend):
    ops, dev, _ = backend
    Y = _y4m().YuvFormat
    p = torch.zeros(128, dtype=torch.uint8, device=dev)
    x = torch.zeros((1, 3, 4, 4), dtype=torch.float32, device=dev)
    for bad in (Y(4, 4, 420, 0, "bt709", 0, 11), Y(5, 4, 420, 0, "bt709", 0, 10), Y(5, 4, 422, 1, "bt709", 0, 10), Y(4, 4, 444, 1, "bt709", 0, 10)):
        with pytest.raises(ValueError):
            ops.yuv_to_planar_f32(p, bad)
        with pytest.raises(ValueError):
            ops.rgb_f32_to_yuv(x, bad)
        with pytest.raises(ValueError):
            ops.luma_grid(p, bad)
    with pytest.raises(ValueError, match="8-bit"):
        ops.yuv_to_rgb_u8(torch.zeros(48, dtype=torch.uint8, device=dev), Y(4, 4, 420, 0, "bt709", 0, 10))
    good = Y(4, 4, 420, 0, "bt709", 0, 10)
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    grid = torch.zeros(4, dtype=torch.int32, device=dev)
    for H, W, ss, sit, B in ((4, 4, 420, 0, 11), (4, 4, 420, 0, 8), (4, 5, 420, 0, 10), (5, 4, 420, 0, 10), (4, 5, 422, 0, 10), (4, 4, 444, 1, 10),
                             (4, 4, 411, 0, 10), (0, 4, 444, 0, 10)):
        with pytest.raises(RuntimeError, match="1001"):                 # the library's own argument check
            ops.lib.call("zt_yuv16_to_planar_f32", p, f, H, W, ss, sit, B, good.decode_coef(), None)
        with pytest.raises(RuntimeError, match="1001"):
            ops.lib.call("zt_rgb_f32_to_yuv16", f, p, H, W, ss, sit, B, good.encode_coef(), None)
    for B in (11, 8, 17):
        with pytest.raises(RuntimeError, match="1001"):
            ops.lib.call("zt_luma_grid_u16", p, 4, 4, B, 16, grid, None)


# ---------------------------------------------------------------------------------------------------- 7. host (no kernels)
def test_header_and_format_depth():
    y = _y4m()
    line = b"YUV4MPEG2 W10 H6 F25:1 Ip C420p10 XCOLORRANGE=LIMITED\n"
    with pytest.raises(ValueError, match="C420p10"):
        y.parse_header(line)
    with pytest.raises(ValueError, match="C420p10"):
        y.parse_header(line, max_depth=8)
    h = y.parse_header(line, max_depth=16)
    assert h.ctag == "420p10" and y.parse_header(h.to_bytes(), max_depth=16) == h
    f = h.format()
    assert f == y.YuvFormat(10, 6, 420, 1, "bt709", 0, 10) and f.depth == 10 and f.frame_bytes == 2 * (60 + 2 * 15)
    assert f._replace(depth=8).frame_bytes == 90
    Y, U, V = f.planes(np.zeros(f.frame_bytes, np.uint8))
    assert Y.dtype.itemsize == 2 and Y.shape == (6, 10) and U.shape == (3, 5) and V.shape == (3, 5)
    for ss in (420, 422, 444):
        for B in (9, 10, 12, 14, 16):
            hh = y.parse_header(b"YUV4MPEG2 W4 H4 C%dp%d\n" % (ss, B), max_depth=16)
            assert hh.format() == y.YuvFormat(4, 4, ss, 0 if ss == 444 else 1, "bt709", 0, B)
    for bad in (b"C420p11", b"C420p8", b"Cmono16", b"Cmono", b"C444alpha", b"C420p10 It"):
        with pytest.raises(ValueError):
            y.parse_header(b"YUV4MPEG2 W4 H4 " + bad + b"\n", max_depth=16)
    with pytest.raises(ValueError, match="W5"):
        y.parse_header(b"YUV4MPEG2 W5 H4 C422p10\n", max_depth=16)
    # the 8-bit format is what it was
    f8 = y.YuvFormat(4, 4, 420, 1, "bt709", 0)
    assert f8.depth == 8 and f8 == y.parse_header(b"YUV4MPEG2 W4 H4 C420mpeg2\n").format() and f8.frame_bytes == 24
    assert f8.decode_coef().dtype == torch.int32 and f.decode_coef().dtype == torch.int64 and f.encode_coef().dtype == torch.int64
    with pytest.raises(ValueError, match="depth"):
        y.YuvFormat(4, 4, 420, 1, "bt709", 0, 11).check()
    # tags across depths
    assert [y.ctag_at_depth(c, 10) for c in ("420jpeg", "420mpeg2", "422", "444", "420p12")] == ["420p10", "420p10", "422p10", "444p10", "420p10"]
    assert [y.ctag_at_depth(c, 8) for c in ("420p10", "422p12", "444p16", "420jpeg")] == ["420mpeg2", "422", "444", "420jpeg"]


def test_encode_host_deep():
    """`encode_host` on uint16 levels is the restated encode"""
    y = _y4m()
    for combo in (COMBOS[0], COMBOS[5], COMBOS[14], COMBOS[19]):
        for B in (10, 16):
            fmt, _, x = case(38, 52, combo, B)
            L16 = quant16(x)
            assert np.array_equal(y.encode_host(L16.astype(np.uint16), fmt), ref_encode16(L16, fmt)[0])
    with pytest.raises(AssertionError):
        y.encode_host(np.zeros((38, 52, 3), np.uint8), fmt)


def _deep_clip(tmp_path, ctag, n=7, W=10, H=6):
    y = _y4m()
    head = y.Header(W, H, "25:1", "p", None, ctag, None)
    rng = np.random.default_rng(6)
    payloads = [rng.integers(0, 256, head.format().frame_bytes, dtype=np.uint8) for _ in range(n)]
    path = tmp_path / ("clip_%s.y4m" % ctag)
    y.write_file(str(path), head, payloads)
    return path, head, payloads


def test_deep_writer_reader_round_trip(tmp_path):
    y = _y4m()
    src, head, payloads = _deep_clip(tmp_path, "422p12")
    assert head.format().frame_bytes == 2 * (60 + 2 * 30)
    path = tmp_path / "w.y4m"
    w = y.Y4MWriter(str(path), head, slots=2)
    for i, p in enumerate(payloads):
        w.submit(p if i % 2 else torch.from_numpy(p))
    w.close()
    assert w.frames == 7 and path.stat().st_size == w.bytes + len(head.to_bytes())
    assert path.read_bytes() == src.read_bytes()
    r = y.Y4MReader(str(path), slots=2, pin=False)
    assert r.header == head and r.frame_bytes == 240
    got = [f.numpy().copy() for f in r]
    assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got, payloads))


def test_deep_reader_truncated_frame_raises(tmp_path):
    y = _y4m()
    src, head, payloads = _deep_clip(tmp_path, "422p12")
    (tmp_path / "cut.y4m").write_bytes(src.read_bytes()[:-121])      # ends inside the last frame, past what 8 bits would need
    r = y.Y4MReader(str(tmp_path / "cut.y4m"), pin=False)
    got = []
    with pytest.raises(ValueError, match="truncated"):
        for f in r:
            got.append(f.numpy().copy())
    assert len(got) == 6 and np.array_equal(got[5], payloads[5])


def test_inferstep_rejects_a_deep_resize():
    infer = importlib.import_module("zero-tig_amd.infer")
    fmt = _y4m().YuvFormat(160, 128, 420, 1, "bt709", 0, 10)
    with pytest.raises(ValueError, match="10-bit"):
        infer.InferStep(None, ingest_size=(1920, 1080), yuv=fmt)
    step = infer.InferStep(None, ingest_size=(160, 128), yuv=fmt)
    assert step.yuv_format == fmt
    assert infer.InferStep(None, ingest_size=None, yuv=fmt, yuv_out_depth=8).yuv_format == fmt._replace(depth=8)
    assert infer.InferStep(None, ingest_size=(1920, 1080), yuv=fmt._replace(depth=8), yuv_out_depth=12).yuv_format == \
        _y4m().YuvFormat(1920, 1080, 420, 1, "bt709", 0, 12)


# -------------------------------------------------------------------------------------------------------- 8. InferStep
def _synth_levels(synth, t, H, W):
    a = np.asarray(synth.lowlight_frame(t, H, W), dtype=np.float32)
    return (np.transpose(a[0] if a.ndim == 4 else a, (1, 2, 0)).astype(np.float64) * 65535.0 + 0.5).astype(np.int64)


def _synth_payload(synth, t, fmt):
    L16 = _synth_levels(synth, t, fmt.H, fmt.W)
    return ref_encode16(L16, fmt)[0] if fmt.depth > 8 else t8.ref_encode((L16 >> 8).astype(np.uint8), fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("ctag,out_depth", [("420p10", None), ("420p10", 8), ("420mpeg2", 10)])
def test_inferstep_yuv_deep(hip_ops, synth, ctag, out_depth):
    """4 frames through InferStep(yuv=, yuv_out_depth=) with the graph, bf16, 128 x 160, of_scale 1 as test_y4m.py's
    test_inferstep_yuv: the step's input is the decode of the payload, both output payloads are the encode of H2 / H3 at the
    output depth, bit for bit; the graph is captured once and replays from the third frame."""
    ops, dev = hip_ops
    H, W = 128, 160
    infer = importlib.import_module("zero-tig_amd.infer")
    fmt = _y4m().Header(W, H, None, None, None, ctag, None).format("bt709")
    step = infer.InferStep(t8._net(ops, dev, synth, "bf16"), use_graph=True, ingest_size=None, yuv=fmt, yuv_out_depth=out_depth)
    out_fmt = fmt._replace(depth=fmt.depth if out_depth is None else out_depth)
    assert step.yuv_format == out_fmt
    for t in range(4):
        payload = _synth_payload(synth, t, fmt)
        out = step(torch.from_numpy(payload.copy()).pin_memory(), is_new_seq=t == 0)
        assert (step.graph is not None) == (t >= 2), t
        assert torch.equal(step.x, ops.yuv_to_planar_f32(torch.from_numpy(payload.copy()).to(dev), fmt)), t
        for i in (0, 1):
            assert step.yuv[i].numel() == out_fmt.frame_bytes
            assert torch.equal(step.yuv[i], ops.rgb_f32_to_yuv(out[i], out_fmt)), (t, i)
    assert step.n_captures == 1


# ---------------------------------------------------------------------------------------------------------- 9. scripts
@pytest.mark.gpu
def test_scripts_y4m_deep(tmp_path, synth):
    y = _y4m()
    n, H, W = 4, 270, 480
    head = y.Header(W, H, "30000:1001", "p", None, "420p10", "LIMITED")
    fmt = head.format("bt709")
    src = tmp_path / "clip_420p10.y4m"
    y.write_file(str(src), head, [_synth_payload(synth, t, fmt) for t in range(n)])
    weights = tmp_path / "weights.pt"
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, str(weights))
    common = ("--model_pretrain", weights, "--graph", "1", "--precision", "bf16", "--of_scale", "1", "--y4m_in", src)
    r = t8._run("predict.py", *common, "--save", tmp_path / "deep")
    assert "10-bit" in r.stdout
    for kind in ("enhance", "denoise"):
        h, frames = t8._frames_of(tmp_path / "deep" / ("clip_420p10_%s.y4m" % kind))
        assert h == head and len(frames) == n and all(f.size == fmt.frame_bytes for f in frames), (kind, h, len(frames))
        assert all(int(f.view("<u2").max()) <= 1023 for f in frames) and any(int(f.view("<u2").max()) > 255 for f in frames)
    t8._run("predict.py", *common, "--save", tmp_path / "flat", "--y4m_out_depth", "8")
    for kind in ("enhance", "denoise"):
        h, frames = t8._frames_of(tmp_path / "flat" / ("clip_420p10_%s.y4m" % kind))
        assert h == head._replace(ctag="420mpeg2") and len(frames) == n and all(f.size == fmt.frame_bytes // 2 for f in frames), (kind, h)
    r = t8._run("predict.py", *common, "--save", tmp_path / "no", "--y4m_resize", "1", ok=False)
    assert r.returncode != 0 and "--y4m_resize" in r.stderr and "--y4m_in" in r.stderr and "10-bit" in r.stderr, (r.returncode, r.stderr[-500:])
    r = t8._run("predict.py", "--model_pretrain", weights, "--save", tmp_path / "no", "--y4m_out_depth", "10", ok=False)
    assert r.returncode != 0 and "--y4m_out_depth" in r.stderr and "--y4m_in" in r.stderr, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "no").exists()
