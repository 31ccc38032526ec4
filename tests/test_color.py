"""zt_color_stats_f32 (csrc/zt_color.hip) through `Ops.color_stats` against a numpy restatement of its definition, on the
host emulator and, under -m gpu, on the MI355X.

Restatement: levels in numpy float32 with one rounding (`rint(v * 255) & 255`); the moments of R - G and R + G - 2B in int64, their
trimmed sums by `np.sort`, the quantiles of the lightness key by the cumulative count; CIELAB through the two tables (made here in
float64 by the formulas, not taken from ops.py) in float32 arrays, one rounding an operation, the three sums in float64; the Sobel
pair on `np.pad(mode="edge")` of the levels in int64, the extrema per block by reshaping; the logarithms in float64.

Anchors of the restatement, each checked once: the trimmed sum from sorting equals the walk over the histogram (heavy ties,
N % 10 != 0); `lin16` and the nine matrix integers are the printed values; grey frames give sum C == 0 exactly.

Gates: the 18 integers equal; the seven floats within SSIM_TOL (1e-9) relative -- the terms are the same fp32 / integer values, what
differs is the order of at most 7e4 fp64 additions and another library's log; a second call gives the same bits; the outputs land
in cells of a table row and nowhere else."""
import numpy as np
import pytest
import torch

from test_metrics import SSIM_TOL

M = np.array([[28440, 24655, 12441], [13938, 46868, 4730], [1164, 7174, 57198]], dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------- restatement
def tables():
    v = np.arange(256, dtype=np.float64) / 255.0
    lin16 = np.rint(65535.0 * np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)).astype(np.int64)
    t = np.arange(65536, dtype=np.float64) / 65535.0
    flut = np.where(t > 216.0 / 24389.0, np.cbrt(t), (24389.0 / 27.0 * t + 16.0) / 116.0).astype(np.float32)
    return lin16, flut


LIN16, FLUT = tables()


def levels(x):
    return np.rint(x.astype(np.float32) * np.float32(255.0)).astype(np.int64) & 255


def trimmed(values):
    """-> (T, n_kept): in ascending order drop the first (N + 9) // 10 and the last N // 10"""
    s = np.sort(values.ravel())
    n = s.size
    tl, tr = (n + 9) // 10, n // 10
    return int(s[tl:n - tr].sum()), n - tl - tr


def trimmed_walk(values, lo):
    """the same by walking the histogram of `values - lo`, as the kernel does"""
    v = values.ravel()
    n = v.size
    tl, hi = (n + 9) // 10, n - n // 10
    h = np.bincount(v - lo)
    incl = np.cumsum(h)
    kept = np.maximum(np.minimum(incl, hi) - np.maximum(incl - h, tl), 0)
    return int((kept * (np.arange(h.size) + lo)).sum())


def lab(lv):
    """levels int64 [3,H,W] -> (C, S, kL): float32, float32, int64, every operation rounded once to float32"""
    r, g, b = (LIN16[c] for c in lv)
    X, Y, Z = ((M[i, 0] * r + M[i, 1] * g + M[i, 2] * b + 32768) >> 16 for i in range(3))
    f32 = np.float32
    fx, fy, fz = FLUT[X], FLUT[Y], FLUT[Z]
    L = f32(116.0) * fy - f32(16.0)
    a = f32(500.0) * (fx - fy)
    bb = f32(200.0) * (fy - fz)
    C = np.sqrt(a * a + bb * bb)
    D = np.sqrt(C * C + L * L)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(D > 0, C / np.where(D > 0, D, f32(1.0)), f32(0.0)).astype(f32)
    assert C.dtype == f32 and D.dtype == f32 and L.dtype == f32
    kL = np.clip(np.floor(L * f32(10.0)).astype(np.int64), 0, 1000)
    return C, S, kL


def sobel_e2(ch):
    """int64 [H,W] levels of one channel -> (gx^2 + gy^2) * c^2, frame borders replicated"""
    p = np.pad(ch, 1, mode="edge")
    H, W = ch.shape
    s = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    return (gx * gx + gy * gy) * ch * ch


def per_block(a, B, fn):
    """[H,W] -> fn over each B x B block, [k2,k1]; the rows and columns left over belong to no block"""
    k2, k1 = a.shape[0] // B, a.shape[1] // B
    return fn(fn(a[:k2 * B, :k1 * B].reshape(k2, B, k1, B), 3), 1)


def restate(x, B):
    """x: float32 [3,H,W] -> (18 integers, 7 floats)"""
    lv = levels(x)
    R, G, Bl = lv
    H, W = R.shape
    N = H * W
    k2, k1 = H // B, W // B
    rg, yb = R - G, R + G - 2 * Bl
    t_rg, kept = trimmed(rg)
    t_yb, _ = trimmed(yb)
    C, S, kL = lab(lv)
    cum = np.cumsum(np.bincount(kL.ravel(), minlength=1001))
    k01, k99 = int(np.argmax(cum >= (N + 99) // 100)), int(np.argmax(cum >= (99 * N + 99) // 100))
    zero_min, E = [], []
    for ch in lv:
        e2 = sobel_e2(ch)
        assert e2.max() < 1 << 37
        hi, lo = per_block(e2, B, np.max), per_block(e2, B, np.min)
        zero_min.append(int((lo == 0).sum()))
        ok = lo > 0
        E.append(float(np.log(hi[ok].astype(np.float64) / lo[ok].astype(np.float64)).sum()))
    cmax = np.max([per_block(ch, B, np.max) for ch in lv], axis=0)
    cmin = np.min([per_block(ch, B, np.min) for ch in lv], axis=0)
    ok = cmax > cmin
    r = (cmax[ok] - cmin[ok]).astype(np.float64) / (cmax[ok] + cmin[ok]).astype(np.float64)
    A = float((r * np.log(r)).sum())
    ints = [N, k1 * k2, int(R.sum()), int(G.sum()), int(Bl.sum()), int(rg.sum()), int((rg * rg).sum()), t_rg,
            int(yb.sum()), int((yb * yb).sum()), t_yb, kept, k01, k99] + zero_min + [int((cmax == cmin).sum())]
    C64 = C.astype(np.float64)
    return ints, [float(C64.sum()), float((C64 * C64).sum()), float(S.astype(np.float64).sum())] + E + [A]


# ------------------------------------------------------------------------------------------------------------------ frames
def make(kind, H, W, seed, synth=None):
    rng = np.random.default_rng(seed)
    lv = lambda a: (np.asarray(a, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    if kind == "uniform":                                   # values below 0 and above 1: the & 255 wrap is part of the definition
        return rng.uniform(-0.3, 1.4, (3, H, W)).astype(np.float32)
    if kind == "grey":                                      # R = G = B noise
        return np.repeat(rng.random((1, H, W)).astype(np.float32), 3, axis=0)
    if kind in ("constant", "tint"):                        # one grey level; one colour: flat in every channel, not across them
        return lv(np.broadcast_to(np.array([90, 90, 90] if kind == "constant" else [200, 90, 31]).reshape(3, 1, 1), (3, H, W)))
    if kind == "black":                                     # D = 0
        return np.zeros((3, H, W), dtype=np.float32)
    if kind == "white":
        return np.ones((3, H, W), dtype=np.float32)
    if kind in ("step90", "step995"):                       # two levels, 90 % / 10 % or 99.5 % / 0.5 % of the pixels, shuffled
        n = H * W
        few = n // 10 if kind == "step90" else max(1, n // 200)
        pick = rng.permutation(n) < few
        a = np.where(pick.reshape(1, H, W), np.array([220, 60, 140]).reshape(3, 1, 1), np.array([30, 70, 20]).reshape(3, 1, 1))
        return lv(a)
    fn = synth.lowlight_frame if kind == "lowlight" else synth.clean_frame
    a = np.asarray(fn(1, H, W, seed), dtype=np.float32)
    return np.ascontiguousarray(a[0] if a.ndim == 4 else a)


def run(ops, dev, x, B, max_workgroups=0):
    """the entry point into cells of a table row, then again into fresh tensors -> (ints, floats); both calls the same bits"""
    tx = torch.from_numpy(x[None].copy()).to(dev)
    tab_i = torch.full((2, 20), -1, dtype=torch.int64, device=dev)
    tab_f = torch.full((2, 9), -1.0, dtype=torch.float64, device=dev)
    oi, of = ops.color_stats(tx, B, out_i=tab_i[1, 1:19], out_f=tab_f[1, 1:8], max_workgroups=max_workgroups)
    assert oi.data_ptr() == tab_i[1, 1:19].data_ptr() and of.data_ptr() == tab_f[1, 1:8].data_ptr()
    ti, tf = tab_i.cpu(), tab_f.cpu()
    assert ti[0].tolist() == [-1] * 20 and ti[1, 0] == -1 and ti[1, 19] == -1
    assert tf[0].tolist() == [-1.0] * 9 and tf[1, 0] == -1.0 and tf[1, 8] == -1.0
    oi2, of2 = ops.color_stats(tx, B, max_workgroups=max_workgroups)
    assert oi2.dtype == torch.int64 and tuple(oi2.shape) == (18,) and of2.dtype == torch.float64 and tuple(of2.shape) == (7,)
    assert oi2.cpu().tolist() == ti[1, 1:19].tolist()
    assert of2.cpu().numpy().tobytes() == tf[1, 1:8].numpy().tobytes()
    return ti[1, 1:19].tolist(), tf[1, 1:8].tolist()


REFS = {}


def reference(kind, H, W, B, synth):
    """the frame and its restatement, computed once and shared by the back-ends"""
    key = (kind, H, W, B)
    if key not in REFS:
        x = make(kind, H, W, 11 + H, synth)
        x.setflags(write=False)
        REFS[key] = (x,) + restate(x, B)
    return REFS[key]


def check(ops, dev, kind, H, W, B, synth, max_workgroups=0):
    x, ints, floats = reference(kind, H, W, B, synth)
    gi, gf = run(ops, dev, x, B, max_workgroups)
    print("ints %r\n ref %r\nfloats %r\n   ref %r" % (gi, ints, gf, floats))
    assert gi == ints
    for g, w in zip(gf, floats):
        assert abs(g - w) <= SSIM_TOL * max(abs(w), 1.0), (g, w)
    return ints, floats


# ------------------------------------------------------------------------------------------------------------------- tests
def test_restatement_anchors():
    assert LIN16[:6].tolist() == [0, 20, 40, 60, 80, 99] and LIN16[253:].tolist() == [64372, 64952, 65535]
    assert M.sum(axis=1).tolist() == [65536] * 3
    assert M.tolist() == [[28440, 24655, 12441], [13938, 46868, 4730], [1164, 7174, 57198]]
    rng = np.random.default_rng(0)
    for n, top in ((1, 3), (7, 2), (23, 3), (101, 2), (999, 5), (1000, 4)):     # heavy ties, N % 10 != 0 and == 0
        v = rng.integers(-top, top + 1, n)
        assert trimmed(v)[0] == trimmed_walk(v, -top), (n, top)
        assert trimmed(v)[1] == n - (n + 9) // 10 - n // 10
    assert trimmed(np.array([5]))[1] == 0 and trimmed(np.array([5]))[0] == 0
    g = np.repeat(np.arange(256, dtype=np.int64).reshape(1, 16, 16), 3, axis=0)
    C, S, _ = lab(g)
    assert float(np.abs(C).max()) == 0.0 and float(np.abs(S).max()) == 0.0   # grey: X16 = Y16 = Z16, a = b = 0 exactly


# size, block, max_workgroups: one pixel (n_kept = 0, nblk = 0); one block with every Sobel tap replicated; one block; remainders
# on both sides, the last block's Sobel reads real pixels beyond it; a small ragged frame; W % 4 == 0 and several bands; the
# smallest and the largest block (64: a block in 16 slices); 33 bands over two workgroups whose tables meet in the same bins
SHAPES = [(1, 1, 10, 0), (4, 4, 4, 0), (10, 10, 10, 0), (23, 37, 10, 0), (38, 52, 10, 0), (136, 200, 10, 0), (136, 200, 8, 0),
          (136, 200, 64, 0), (330, 12, 10, 2)]
SHAPE_IDS = ["%dx%d-B%d-wg%d" % s for s in SHAPES]


@pytest.mark.parametrize("kind", ["uniform", "grey"])
@pytest.mark.parametrize("H,W,B,wg", SHAPES, ids=SHAPE_IDS)
def test_shapes(backend, synth, H, W, B, wg, kind):
    ops, dev, _ = backend
    ints, floats = check(ops, dev, kind, H, W, B, synth, wg)
    assert ints[0] == H * W and ints[1] == (H // B) * (W // B)
    if H * W == 1:
        assert ints[11] == 0 and ints[7] == 0 and ints[10] == 0
    if kind == "grey":
        assert floats[0] == 0.0 and floats[1] == 0.0 and floats[2] == 0.0 and ints[5:11] == [0] * 6


@pytest.mark.parametrize("kind", ["constant", "black", "white", "tint"])
@pytest.mark.parametrize("H,W,B,wg", [(23, 37, 10, 0), (330, 12, 10, 2)], ids=["23x37", "330x12-wg2"])
def test_flat_frames(backend, synth, H, W, B, wg, kind):
    """every block flat: every E and A zero, all four block counters equal nblk; black has D = 0; one colour ("tint") has no
    edge either, but its three levels differ, so every block adds the same r ln r"""
    ops, dev, _ = backend
    ints, floats = check(ops, dev, kind, H, W, B, synth, wg)
    nblk = (H // B) * (W // B)
    assert ints[14:17] == [nblk] * 3 and floats[3:6] == [0.0] * 3
    if kind == "tint":
        assert ints[17] == 0 and floats[6] < 0.0 and floats[0] > 0.0
        return
    assert ints[17] == nblk and floats[6] == 0.0
    if kind in ("black", "white"):
        assert floats[0:3] == [0.0] * 3 and ints[12] == ints[13] == (0 if kind == "black" else 1000)


@pytest.mark.parametrize("kind", ["step90", "step995"])
@pytest.mark.parametrize("H,W", [(38, 52), (40, 50)], ids=["38x52", "40x50"])
def test_two_levels(backend, synth, H, W, kind):
    """the quantiles and the trim boundaries fall on and beside a step (N % 10 != 0 and == 0)"""
    ops, dev, _ = backend
    ints, _ = check(ops, dev, kind, H, W, 10, synth)
    assert ints[12] < ints[13] if kind == "step90" else ints[12] == ints[13]


@pytest.mark.parametrize("kind", ["lowlight", "clean"])
def test_synthetic_frames(backend, synth, kind):
    """the project's own frames at 136 x 200: some blocks have a zero Sobel minimum, far from all, and no block is flat"""
    ops, dev, _ = backend
    ints, floats = check(ops, dev, kind, 136, 200, 10, synth)
    nblk = ints[1]
    assert nblk == 13 * 20 and all(v < nblk for v in ints[14:17]) and ints[17] == 0
    assert all(v > 0.0 for v in floats[3:6]) and floats[6] < 0.0


def test_ops_asserts(backend):
    ops, dev, _ = backend
    a = torch.zeros((1, 3, 6, 8), dtype=torch.float32, device=dev)
    bad = [(a.double(), 10), (a[0], 10), (a[:, :1], 10), (a.permute(0, 1, 3, 2), 10), (a, 3), (a, 65), (a, 10.5)]
    for x, block in bad:
        with pytest.raises(AssertionError):
            ops.color_stats(x, block)
    with pytest.raises(AssertionError):
        ops.color_stats(a, max_workgroups=-1)
    with pytest.raises(AssertionError):
        ops.color_stats(a, out_i=torch.zeros(18, dtype=torch.int32, device=dev))
    with pytest.raises(AssertionError):
        ops.color_stats(a, out_f=torch.zeros(6, dtype=torch.float64, device=dev))
