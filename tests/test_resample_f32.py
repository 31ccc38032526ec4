"""The float resize: `zt_resample_planar_f32` / `Ops.resize_planar_f32` against the definition restated here in numpy
(float64 accumulation in tap order, rounded to float32 after each pass, with its own restatement of Pillow's coefficient table) bit
for bit, and against Pillow's own mode-F BICUBIC resize; the clamp, the argument checks, and `Ops.yuv_to_planar_f32_sized`."""
import importlib
import math

import numpy as np
import pytest
import torch
from PIL import Image

# (Hin, Win) -> (Hout, Wout)
SHAPES = [((38, 52), (19, 26)),         # exact 2:1
          ((54, 96), (27, 50)),         # non-integer ratio, ksize differs per axis
          ((20, 24), (33, 41)),         # upscale: filterscale clamps to 1
          ((17, 258), (9, 100)),        # wide source row
          ((9, 100), (17, 258)),        # output rows wider than one block of 256 threads, in both passes
          ((2, 2), (5, 3)),             # tiny
          ((24, 200), (24, 77)),        # horizontal pass only
          ((24, 200), (11, 200))]       # vertical pass only
IDS = ["%dx%d-%dx%d" % (a + b) for a, b in SHAPES]


def _ingest():
    return importlib.import_module("zero-tig_amd.ingest")


def _y4m():
    return importlib.import_module("zero-tig_amd.y4m")


# ---------------------------------------------------------------------------------------- the definition, restated
def _cubic(x):
    x = abs(x)
    if x < 1.0:
        return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * -0.5
    return 0.0


def ref_table(n_in, n_out):
    """Pillow's precompute_coeffs for BICUBIC: per output sample (first, [weights]) in double precision"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    rows = []
    for o in range(n_out):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [_cubic((x - center + 0.5) * (1.0 / fs)) for x in range(lo, hi)]
        tot = 0.0
        for v in w:
            tot += v
        rows.append((lo, [v / tot for v in w] if tot != 0.0 else w))
    return rows, int(math.ceil(support)) * 2 + 1


def ref_pass(a, n_out, axis):
    """one pass over float32 [C][H][W] along `axis` (1 = H, 2 = W): float64 sums in tap order, one rounding to float32"""
    a = np.moveaxis(np.asarray(a, dtype=np.float32), axis, -1)
    rows, _ = ref_table(a.shape[-1], n_out)
    out = np.empty(a.shape[:-1] + (n_out,), np.float32)
    for o, (lo, w) in enumerate(rows):
        ss = np.zeros(a.shape[:-1], np.float64)
        for t, c in enumerate(w):
            ss = ss + a[..., lo + t].astype(np.float64) * np.float64(c)
        out[..., o] = ss.astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(out, -1, axis))


def ref_resize(a, Ho, Wo):
    """[C][H][W] -> [C][Ho][Wo]: horizontal pass, then vertical; an unchanged axis is skipped"""
    a = np.asarray(a, dtype=np.float32)
    if a.shape[2] != Wo:
        a = ref_pass(a, Wo, 2)
    if a.shape[1] != Ho:
        a = ref_pass(a, Ho, 1)
    return a


def _planes(C, H, W, seed=3):
    return np.random.default_rng(seed).random((C, H, W), dtype=np.float32)


_REF = {}


def _case(C, src, dst):
    """input and the unclamped reference, computed once and left unchanged"""
    key = (C, src, dst)
    if key not in _REF:
        x = _planes(C, *src)
        ref = ref_resize(x, *dst)
        x.setflags(write=False), ref.setflags(write=False)
        _REF[key] = (x, ref)
    return _REF[key]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


# ------------------------------------------------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("n_in,n_out", [(52, 26), (96, 50), (24, 41), (258, 100), (2, 5), (3840, 1920)])
def test_tables(n_in, n_out):
    ing = _ingest()
    coef, bounds, ks = ing.pil_bicubic_tables_f64(n_in, n_out)
    rows, ks_ref = ref_table(n_in, n_out)
    assert coef.dtype == np.float64 and coef.shape == (n_out, ks) and bounds.dtype == np.int32 and bounds.shape == (n_out, 2) and ks == ks_ref
    for o, (lo, w) in enumerate(rows):
        assert tuple(bounds[o]) == (lo, len(w)) and len(w) <= ks and lo + len(w) <= n_in
        assert np.array_equal(coef[o, :len(w)], np.array(w, np.float64)) and not coef[o, len(w):].any()
        assert abs(math.fsum(w) - 1.0) <= 4 * 2.0 ** -52 * len(w)
    # the windows are those of the 8-bit table; its integers are these weights, rounded
    ci, bi, ki = ing.pil_bicubic_tables(n_in, n_out)
    assert ki == ks and np.array_equal(bi, bounds)
    assert np.abs(ci - coef * 2.0 ** ing.PRECISION_BITS).max() <= 0.5 + 1e-6


# ----------------------------------------------------------------------------------- 2. the definition and Pillow, bit for bit
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_resize_definition_and_pillow(backend, src, dst, C):
    ops, dev, _ = backend
    x, ref = _case(C, src, dst)
    got = ops.resize_planar_f32(_dev(x, dev)[None], (dst[1], dst[0]), clamp=False)
    assert tuple(got.shape) == (1, C) + dst and got.dtype == torch.float32
    got = got.cpu().numpy()[0]
    assert np.array_equal(got, ref), np.abs(got.astype(np.float64) - ref).max()
    pil = np.stack([np.asarray(Image.fromarray(np.array(x[c]), mode="F").resize((dst[1], dst[0]), Image.BICUBIC)) for c in range(C)])
    err = np.abs(got.astype(np.float64) - pil.astype(np.float64)).max()
    print("resize %s C=%d max |kernel - Pillow| = %.3g" % (IDS[SHAPES.index((src, dst))], C, err))
    # one float ulp for |v| < 2: a Pillow build that contracts the multiply-add may differ by one final rounding
    assert np.abs(pil).max() < 2 and err <= 2.0 ** -22, err


def test_resize_buffers_and_identity(backend):
    """`out` / `tmp` are used as given; both sizes unchanged: the input itself, or a copy into `out`"""
    ops, dev, _ = backend
    x, ref = _case(3, (54, 96), (27, 50))
    xd = _dev(x, dev)[None]
    out = torch.full((1, 3, 27, 50), -7.0, device=dev)
    tmp = torch.full((1, 3, 54, 50), -7.0, device=dev)
    got = ops.resize_planar_f32(xd, (50, 27), clamp=False, out=out, tmp=tmp)
    assert got is out and np.array_equal(out.cpu().numpy()[0], ref)
    assert np.array_equal(tmp.cpu().numpy()[0], ref_pass(x, 50, 2))
    assert ops.resize_planar_f32(xd, (96, 54)) is xd
    same = torch.zeros_like(xd)
    assert ops.resize_planar_f32(xd, (96, 54), out=same) is same and torch.equal(same, xd)
    with pytest.raises(AssertionError):
        ops.resize_planar_f32(xd, (50, 27), out=torch.zeros((1, 3, 27, 51), device=dev))


# ------------------------------------------------------------------------------------------------------------ 3. the clamp
@pytest.mark.parametrize("src,dst", [((20, 24), (33, 41)), ((24, 200), (24, 77)), ((24, 200), (11, 200))], ids=["both", "rows", "columns"])
def test_clamp(backend, src, dst):
    """the clamp sits in the last pass that runs and nowhere else: the result is clip(unclamped reference) bit for bit"""
    ops, dev, _ = backend
    x, ref = _case(3, src, dst)
    if src == (20, 24):                             # the upscale of uniform noise overshoots on both sides: the clamp is exercised
        assert ref.min() < 0 and ref.max() > 1, (ref.min(), ref.max())
    got = ops.resize_planar_f32(_dev(x, dev)[None], (dst[1], dst[0]), clamp=True).cpu().numpy()[0]
    assert np.array_equal(got, np.clip(ref, np.float32(0), np.float32(1)))
    assert got.min() >= 0 and got.max() <= 1


def test_constant_plane(backend):
    """the weights of a row sum to 1 to within rounding: a flat plane stays flat"""
    ops, dev, _ = backend
    for src, dst in SHAPES:
        x = torch.full((1, 1) + src, 0.25, dtype=torch.float32, device=dev)
        got = ops.resize_planar_f32(x, (dst[1], dst[0]), clamp=True).cpu().numpy()
        assert np.abs(got.astype(np.float64) - 0.25).max() <= 2.0 ** -24, (src, dst)


# ------------------------------------------------------------------------------------------------------------ 4. arguments
def test_argument_errors(backend):
    ops, dev, _ = backend
    coef, bounds, ks = _ingest().pil_bicubic_tables_f64(8, 4)
    coef, bounds = _dev(coef, dev), _dev(bounds, dev)
    src = torch.zeros((2, 6, 8), dtype=torch.float32, device=dev)
    dst = torch.zeros((2, 6, 4), dtype=torch.float32, device=dev)
    good = dict(src=src, dst=dst, C=2, Hi=6, Wi=8, No=4, axis=1, coef=coef, bounds=bounds, ksize=ks)

    def call(**kw):
        a = dict(good, **kw)
        ops.lib.call("zt_resample_planar_f32", a["src"], a["dst"], a["C"], a["Hi"], a["Wi"], a["No"], a["axis"], a["coef"], a["bounds"],
                     a["ksize"], 0, None)
    call()
    for bad in (dict(src=None), dict(dst=None), dict(coef=None), dict(bounds=None), dict(C=0), dict(Hi=0), dict(Wi=-1), dict(No=0),
                dict(axis=2), dict(axis=-1), dict(ksize=0), dict(dst=src)):
        with pytest.raises(RuntimeError, match="1001"):
            call(**bad)


# ------------------------------------------------------------------------------------------------ 5. decode + resize in one call
@pytest.mark.parametrize("ctag", ["420mpeg2", "444p10"])
def test_yuv_to_planar_f32_sized(backend, ctag):
    ops, dev, _ = backend
    y = _y4m()
    H, W, Ho, Wo = 38, 52, 26, 20
    fmt = y.Header(W, H, None, None, None, ctag, None).format("bt709")
    rng = np.random.default_rng(11)
    bufs = ops.sized_bufs(fmt, (Wo, Ho), dev)
    ptrs = {k: v.data_ptr() for k, v in bufs.items() if v is not None}
    out = torch.empty((1, 3, Ho, Wo), dtype=torch.float32, device=dev)
    for _ in range(2):                              # the buffers are reused: same addresses, new contents
        if fmt.depth > 8:
            payload = rng.integers(0, 1 << fmt.depth, fmt.frame_bytes // 2).astype("<u2").view(np.uint8)
        else:
            payload = rng.integers(0, 256, fmt.frame_bytes, dtype=np.uint8)
        p = _dev(payload, dev)
        full = ops.yuv_to_planar_f32(p, fmt)
        want = ops.resize_planar_f32(full, (Wo, Ho))
        got = ops.yuv_to_planar_f32_sized(p, fmt, (Wo, Ho), out=out, bufs=bufs)
        assert got is out and torch.equal(got, want) and torch.equal(bufs["decode"], full)
        assert {k: v.data_ptr() for k, v in bufs.items() if v is not None} == ptrs
        assert torch.equal(ops.yuv_to_planar_f32_sized(p, fmt, (Wo, Ho)), want)
        assert float(got.min()) >= 0 and float(got.max()) <= 1
        # against the restated definition as well
        assert np.array_equal(got.cpu().numpy()[0], np.clip(ref_resize(full.cpu().numpy()[0], Ho, Wo), np.float32(0), np.float32(1)))
