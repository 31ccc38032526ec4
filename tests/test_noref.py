"""zt_lightness_joint_hist_f32 / zt_noref_from_hist (csrc/zt_noref.hip) against a numpy restatement of their definition,
on the host emulator and, under -m gpu, on the MI355X.

Restatement: levels and lightness in numpy float32 with one rounding each (`rint(v * 255) & 255`, max over the channels), the joint
histogram by `np.add.at`, the six integers by the cumulative-sum formula in int64, the entropies in float64 in level order.  The
formula's S_loe is itself held against the O(N^2) definition -- the number of ordered sample pairs (p, q) with
(La_p >= La_q) xor (Lb_p >= Lb_q) -- at every size up to 38 x 52, so the restatement is anchored.

Gates: histogram equal, the six integers equal, the entropies within SSIM_TOL relative (256 fp64 terms in a fixed order plus a
log2 of another library), a second call gives the same bits."""
import numpy as np
import pytest
import torch

from test_metrics import SSIM_TOL

CAP = 65535                                                 # what a 16-bit counter of the kernel's private table can hold


# ------------------------------------------------------------------------------------------------------------- restatement
def levels(x):
    return np.rint(x.astype(np.float32) * np.float32(255.0)).astype(np.int64) & 255


def grid_index(n, ns):
    return ((2 * np.arange(ns, dtype=np.int64) + 1) * n) // (2 * ns)


def lightness(a, b, grid=None):
    """a, b: float32 [3,H,W] -> (La, Lb), int64 [Hs,Ws] on the sample grid"""
    H, W = a.shape[1:]
    Hs, Ws = grid or (H, W)
    rows, cols = grid_index(H, Hs), grid_index(W, Ws)
    return tuple(levels(x).max(axis=0)[rows][:, cols] for x in (a, b))


def joint_hist(La, Lb):
    hist = np.zeros((256, 256), dtype=np.int64)
    np.add.at(hist, (La.ravel(), Lb.ravel()), 1)
    return hist


def entropy(h, ns):
    e = 0.0
    for v in h.tolist():
        if v:
            p = np.float64(v) / np.float64(ns)
            e -= p * np.log2(p)
    return float(e)


def from_hist(hist):
    """-> ([Ns, S_loe, S_a, S_b, n_sat, n_black], [E_a, E_b]) by the cumulative-sum formula"""
    C = hist.cumsum(axis=0).cumsum(axis=1)
    R, K = C[:, 255], C[255, :]
    RD = R[:, None] + K[None, :] - 2 * C
    ha, hb = hist.sum(axis=1), hist.sum(axis=0)
    ns = int(hist.sum())
    lev = np.arange(256, dtype=np.int64)
    ints = [ns, int((hist * RD).sum()), int((lev * ha).sum()), int((lev * hb).sum()), int(hb[255]), int(hb[0])]
    return ints, [entropy(ha, ns), entropy(hb, ns)]


def loe_brute(La, Lb):
    la, lb = La.ravel(), Lb.ravel()
    return int(((la[:, None] >= la[None, :]) ^ (lb[:, None] >= lb[None, :])).sum())


# ------------------------------------------------------------------------------------------------------------------ frames
def frame_of(L, rng):
    """a float32 [3,H,W] frame of levels k / 255 whose lightness is the level array L: one channel carries L, the others less"""
    lo = (rng.random((2,) + L.shape) * (L + 1)).astype(np.int64)
    ch = np.stack([lo[0], L, lo[1]])
    return (ch.astype(np.float32) / np.float32(255.0)).astype(np.float32)


def make(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":                                   # values below 0 and above 1: the & 255 wrap is part of the definition
        return tuple(rng.uniform(-0.3, 1.4, (3, H, W)).astype(np.float32) for _ in range(2))
    if kind == "identical":
        a = rng.random((3, H, W)).astype(np.float32)
        return a, a.copy()
    if kind == "dark":                                      # the workload's own contention pattern: a handful of La levels
        return frame_of(rng.integers(0, 13, (H, W)), rng), rng.random((3, H, W)).astype(np.float32)
    if kind == "constant":
        return frame_of(np.full((H, W), 9), rng), frame_of(np.full((H, W), 200), rng)
    if kind == "halves":                                    # Lb alternates between 2k and 2k + 1: both halves of one dword fill
        return frame_of(np.full((H, W), 9), rng), frame_of(200 + (np.arange(H * W).reshape(H, W) & 1), rng)
    La = rng.integers(0, 101, (H, W)) if kind == "increasing" else rng.integers(0, 256, (H, W))
    Lb = {"increasing": 2 * La + 5, "merged": La // 8 * 8, "reversed": 255 - La}[kind]
    return frame_of(La, rng), frame_of(Lb, rng)


def run(ops, dev, a, b, grid=None):
    """both entry points, twice -> (hist int64 [256,256], ints, floats); the second call must give the same bits"""
    ta, tb = (torch.from_numpy(x[None].copy()).to(dev) for x in (a, b))
    hist = ops.lightness_joint_hist(ta, tb, grid)
    assert hist.dtype == torch.uint32 and tuple(hist.shape) == (256, 256)
    tab_i = torch.full((2, 8), -1, dtype=torch.int64, device=dev)       # a row of a table, as evals.py passes it
    tab_f = torch.full((2, 4), -1.0, dtype=torch.float64, device=dev)
    oi, of = ops.noref(ta, tb, grid, out_i=tab_i[1, 1:7], out_f=tab_f[1, 1:3])
    assert oi.data_ptr() == tab_i[1, 1:7].data_ptr() and of.data_ptr() == tab_f[1, 1:3].data_ptr()
    ti, tf = tab_i.cpu(), tab_f.cpu()
    assert ti[0].tolist() == [-1] * 8 and ti[1, 0] == -1 and ti[1, 7] == -1
    assert tf[0].tolist() == [-1.0] * 4 and tf[1, 0] == -1.0 and tf[1, 3] == -1.0
    h = hist.cpu().numpy().astype(np.int64)
    oi2, of2 = ops.noref(ta, tb, grid)
    assert np.array_equal(ops.lightness_joint_hist(ta, tb, grid).cpu().numpy().astype(np.int64), h)
    assert oi2.cpu().tolist() == ti[1, 1:7].tolist()
    assert of2.cpu().numpy().tobytes() == tf[1, 1:3].numpy().tobytes()
    return h, ti[1, 1:7].tolist(), tf[1, 1:3].tolist()


def check(ops, dev, a, b, grid=None, brute=False):
    La, Lb = lightness(a, b, grid)
    want = joint_hist(La, Lb)
    ints, ents = from_hist(want)
    if brute:
        assert ints[1] == loe_brute(La, Lb), (ints[1], loe_brute(La, Lb))
    hist, gi, gf = run(ops, dev, a, b, grid)
    print("ints %r ref %r, entropies %r ref %r" % (gi, ints, gf, ents))
    assert np.array_equal(hist, want), np.argwhere(hist != want)[:8]
    assert gi == ints
    for g, w in zip(gf, ents):
        assert abs(g - w) <= SSIM_TOL * max(abs(w), 1.0), (g, w)
    return ints, ents


# ------------------------------------------------------------------------------------------------------------------- tests
SIZES = [(1, 1), (5, 7), (38, 52), (136, 200), (264, 256)]  # one sample; tails in both axes and scalar loads (W % 4 != 0 twice);
                                                            # 16-byte loads; 67584 samples: two workgroups' flushes meet in the bins
KINDS = ["uniform", "dark", "identical", "increasing", "merged", "reversed"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_full_grid(backend, H, W, kind):
    ops, dev, _ = backend
    a, b = make(kind, H, W, 11 + H)
    ints, ents = check(ops, dev, a, b, brute=H * W <= 38 * 52)
    assert ints[0] == H * W
    if kind in ("identical", "increasing") or H * W == 1:  # the order is kept (ties on both sides alike): nothing flips
        assert ints[1] == 0
    if kind in ("merged", "reversed") and H * W >= 35:      # ties on one side only count: >= against >
        assert ints[1] > 0
    if kind == "identical":
        assert ints[2] == ints[3] and ents[0] == ents[1]
    if kind == "dark":
        assert ints[2] <= 12 * H * W


@pytest.mark.parametrize("kind", ["constant", "halves"])
@pytest.mark.parametrize("H,W", [(256, 256), (264, 256)], ids=["65536", "67584"])
def test_one_bin_past_the_counter(backend, H, W, kind):
    """65536 and 67584 samples in one bin (or in the two halves of one dword): more than a 16-bit counter holds, so a workgroup that
    took them all would wrap its counter to zero or carry into the neighbouring bin"""
    ops, dev, _ = backend
    assert H * W > CAP
    a, b = make(kind, H, W, 3)
    ints, _ = check(ops, dev, a, b)
    assert ints[0] == H * W and ints[4] == 0 and ints[5] == 0
    if kind == "constant":
        assert ints[1] == 0 and ints[2] == 9 * H * W and ints[3] == 200 * H * W


@pytest.mark.parametrize("H,W,grid", [(38, 52, (50, 68)), (136, 200, (50, 74)), (5, 7, (1, 1))],
                         ids=["38x52-on-50x68", "136x200-on-50x74", "5x7-on-1x1"])
def test_sampled_grid(backend, H, W, grid):
    """(50, 68) on 38 x 52 upsamples and repeats pixels; (1, 1) is the centre pixel"""
    ops, dev, _ = backend
    a, b = make("uniform", H, W, 5)
    ints, _ = check(ops, dev, a, b, grid=grid, brute=True)
    assert ints[0] == grid[0] * grid[1]


def test_sampled_grid_over_two_workgroups(backend):
    """300 x 300 samples of a 4 x 4 frame: 90000 > 65535, and two bins take them all"""
    ops, dev, _ = backend
    rng = np.random.default_rng(1)
    a = frame_of(np.full((4, 4), 7), rng)
    b = frame_of(20 + (np.arange(16).reshape(4, 4) & 1), rng)
    G = 300
    assert G * G > CAP
    odd = int((grid_index(4, G) & 1).sum())
    ints, _ = check(ops, dev, a, b, grid=(G, G))
    assert ints[0] == G * G and ints[3] == 20 * G * G + G * odd


def test_ops_asserts(backend):
    ops, dev, _ = backend
    a = torch.zeros((1, 3, 6, 8), dtype=torch.float32, device=dev)
    ok = ops.noref(a, a)
    assert ok[0].dtype == torch.int64 and tuple(ok[0].shape) == (6,) and ok[1].dtype == torch.float64 and tuple(ok[1].shape) == (2,)
    bad = [
        (a.double(), a, None),                                                          # dtype
        (a, a.double(), None),
        (a[0], a[0], None),                                                             # shape
        (a[:, :1], a[:, :1], None),
        (a, torch.zeros((1, 3, 6, 9), dtype=torch.float32, device=dev), None),
        (a.permute(0, 1, 3, 2), a.permute(0, 1, 3, 2), None),                           # not contiguous
        (a, a, (0, 5)), (a, a, (5, 0)), (a, a, (-1, 5)), (a, a, (5,)), (a, a, (2.5, 5)),  # grid
        (a, a, (1 << 16, 1 << 16)),
    ]
    for x, y, grid in bad:
        for fn in (ops.noref, ops.lightness_joint_hist):
            with pytest.raises(AssertionError):
                fn(x, y, grid)
    with pytest.raises(AssertionError):
        ops.noref(a, a, out_i=torch.zeros(6, dtype=torch.int32, device=dev))
    with pytest.raises(AssertionError):
        ops.noref(a, a, out_f=torch.zeros(3, dtype=torch.float64, device=dev))
