"""The weight-gradient family -- wgrad_mfma_bf16_kernel / wgrad64_dma_bf16_kernel and the two slab reductions (zt_wgrad.hip), the
fp32 wgrad_mfma_f32_kernel (zt_conv_f32.hip), thin1x1_bwd_bf16_kernel (zt_conv_thin.hip) and the batched weight repack
(zt_conv.hip) -- with SMALL-INTEGER operands, bit for bit against float64.

K of these GEMMs is the pixel count, so a bound derived from the number formats, (n + 2) 2^-23 sum |x||dz|, sits some forty
thousand times above the real error (worst err / bound 2.3e-5 on these shapes) and is as large as one dropped pixel's whole
contribution.  The kernels fail through exactly such errors: a missed DMA wait, a stale LDS buffer, a wrong tile in the banded
order, a ragged-edge pixel taken twice.  With x, dz, the masks and the initial gradients integers in [-4, 4] every product and
every partial sum is an integer of magnitude <= 16 P + 4 (P = pixels summed into one gradient element); below 2^24 such a sum is
exact in fp32 in ANY order, so each kernel must reproduce the float64 reference exactly: tolerance zero, nothing measured.
`_exact_ok` asserts the condition from each case's own shapes; it decides correctness and is not a tolerance.

The schedule (tiles per workgroup, tile order, slab offsets) is varied through ZT_WGRAD_BLOCKS, ZT_WGRAD_DMA and the size of the
slab handed in (the entry points clamp the workgroup count to it); slab tensors start as NaN, so a slab that is reduced but was
never written poisons the result, and the padding channel slots of every NHWC operand hold 1000 (NaN in one thin-input case).
Every case prints a `WGRADEXACT <case> slabs=<n> depth=<tiles per workgroup> exact=1` line."""
import zlib
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

U8, U23 = 2.0 ** -8, 2.0 ** -23
NAN = float("nan")


def _cv():
    return import_module("zero-tig_amd.ops").CV


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(g, *shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _exact_ok(npix, nadd=1):
    """every partial sum of `npix` products of two integers in [-4, 4], plus an initial gradient in [-4, 4], is an fp32 integer"""
    assert 16 * npix * nadd + 4 < 2 ** 24, npix


def _nhwc(t, ld, fill=1000.0, dtype=torch.bfloat16):
    """NCHW -> NHWC with ld channel slots; the padding slots hold `fill` (they are not the layer's: garbage)"""
    n = t.permute(0, 2, 3, 1)
    out = torch.full((*n.shape[:3], ld), fill)
    out[..., :n.shape[-1]] = n
    return out.to(dtype).contiguous()


def _assert_exact(got, want, what):
    """got == want (float64) bit for bit; otherwise say how many elements differ, by how much, and where the first one is"""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    first = tuple(int(i) for i in bad.nonzero()[0])
    diff = (got - want)[bad]
    finite = diff[torch.isfinite(diff)]
    raise AssertionError("%s: %d of %d elements differ, %d not finite, largest finite difference %g, first at %s %s: got %r, expected %r"
                         % (what, int(bad.sum()), bad.numel(), int(diff.numel() - finite.numel()),
                            float(finite.abs().max()) if finite.numel() else 0.0,
                            "(co, ci, ky, kx)" if got.dim() == 4 else "(co,)", first, float(got[first]), float(want[first])))


def _report(case, slabs, depth):
    print("WGRADEXACT %s slabs=%s depth=%s exact=1" % (case, slabs, depth))


def _wgrad_ref(x, dz, K):
    """float64 autograd of conv2d(x, w) * dz -> (grad_w [Cout, Cin, K, K], grad_b [Cout])"""
    w = torch.zeros(dz.shape[1], x.shape[1], K, K, dtype=torch.float64, requires_grad=True)
    (F.conv2d(x.double(), w, None, padding=K // 2) * dz.double()).sum().backward()
    return w.grad, dz.double().sum(dim=(0, 2, 3))


def _set_env(monkeypatch, dma=None, blocks=None):
    for key, val in (("ZT_WGRAD_DMA", dma), ("ZT_WGRAD_BLOCKS", blocks)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))


def _cdiv(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------------------------------------------------------------
# A. bf16 partial kernels through the deferred path: wgrad_partial_bf16 appended call after call, one wgrad_reduce_multi
# ---------------------------------------------------------------------------------------------------------------------------------
# id -> Cin, ldx, Cout, lddz, K, ZT_WGRAD_DMA, relu mask, 8-wave kernel (8 x 32 tiles, 256 workgroups; else 4 x 32, 512), x padding
LAYERS = {
    "c64-64_dma":      (64, 72, 64, 64, 3, "1", False, True, 1000.0),      # wgrad64_dma_bf16_kernel<64, 64>
    "c64-64_reg":      (64, 72, 64, 64, 3, "0", False, True, 1000.0),      # wgrad_mfma_bf16_kernel<3, 3, 4, 4, 8>
    "c48-48_dma":      (48, 48, 48, 56, 3, "1", False, True, 1000.0),      # wgrad64_dma_bf16_kernel<48, 48>
    "c48-48_reg":      (48, 48, 48, 56, 3, "0", False, False, 1000.0),     # <3, 3, 3, 3, 4>, interior fast path
    "c3-48_ld8_dma":   (3, 8, 48, 48, 3, "1", False, True, NAN),           # wgrad64_dma_bf16_kernel<8, 48>; NaN lanes -> ignored rows
    "c12-48_ld16_dma": (12, 16, 48, 48, 3, "1", False, True, 1000.0),      # wgrad64_dma_bf16_kernel<16, 48>
    "c12-48_ld24_reg": (12, 24, 48, 48, 3, None, False, False, 1000.0),    # pixels not 8 / 16 wide: <3, 3, 1, 3, 4>
    "c9-64":           (9, 16, 64, 64, 3, None, False, False, 1000.0),     # <3, 3, 1, 4, 4>
    "c9-64_mask":      (9, 16, 64, 64, 3, None, True, False, 1000.0),      # <3, 3, 1, 4, 4, MASK>
    "c12-64":          (12, 16, 64, 64, 3, None, False, False, 1000.0),
    "c12-64_mask":     (12, 16, 64, 64, 3, None, True, False, 1000.0),
    "c40-40_ld40":     (40, 40, 40, 40, 3, None, False, False, 1000.0),    # FASTP kernel, interior-tile test AND channel masks
    "c40-40_ld48":     (40, 48, 40, 48, 3, None, False, False, 1000.0),
    "c48-3_k1":        (48, 48, 3, 8, 1, None, False, False, 1000.0),      # <1, 1, 3, 1, 4>
    "c48-6_k1":        (48, 48, 6, 8, 1, None, False, False, 1000.0),
    "c64-3":           (64, 64, 3, 8, 3, None, False, False, 1000.0),      # <3, 3, 4, 1, 4>
}
# 8 x 32 tiles: 43 x 70 = 18 tiles in 6 tile rows (one full band of 4, a ragged band of 2); 4 x 32 tiles: 27 x 101 = 28 tiles
IMAGES8, IMAGES4 = [(43, 70), (16, 129)], [(27, 101), (9, 41)]
# a single pixel, exactly one 8 x 32 tile, one row / column over and under it
EDGES = [(1, 1), (8, 32), (9, 33), (7, 31), (3, 33)]
# default: one tile per workgroup; 1: every tile through both LDS buffers in turn; 3: plain order; 8, 16: the XCD-banded order
# (at 16 some workgroups get two tiles, others one); slab5: 5 workgroups imposed through the slab size (plain order, depth 3-6)
SCHEDULES = ["default", "b1", "b3", "b8", "b16", "slab5"]

_CACHE = {}


def _layer_data(lid, images):
    """integer operands, initial gradients and the float64 reference of one layer over a list of images: built once, shared by
    every schedule and both back-ends, never modified"""
    key = (lid, tuple(images))
    if key in _CACHE:
        return _CACHE[key]
    Cin, ldx, Cout, lddz, K, _, masked, _, xfill = LAYERS[lid]
    g = _gen(lid + repr(images))
    _exact_ok(sum(h * w for h, w in images))
    calls, ref_w, ref_b = [], 0, 0
    for (H, W) in images:
        x, dz = _ints(g, 1, Cin, H, W), _ints(g, 1, Cout, H, W)
        act = torch.relu(_ints(g, 1, Cout, H, W)) if masked else None          # about half the entries exactly zero
        rw, rb = _wgrad_ref(x, dz * (act > 0) if masked else dz, K)
        ref_w, ref_b = ref_w + rw, ref_b + rb
        calls.append((_nhwc(x, ldx, xfill), _nhwc(dz, lddz), _nhwc(act, 72) if masked else None, H, W))
    gw0, gb0 = _ints(g, Cout, Cin, K, K), _ints(g, Cout)
    _CACHE[key] = dict(calls=calls, gw0=gw0, gb0=gb0, want_w=gw0.double() + ref_w, want_b=gb0.double() + ref_b)
    return _CACHE[key]


def _deferred(backend, monkeypatch, lid, images, sched):
    ops, dev, bname = backend
    CV = _cv()
    Cin, ldx, Cout, lddz, K, dma, masked, nw8, _ = LAYERS[lid]
    d = _layer_data(lid, images)
    blocks = int(sched[1:]) if sched[0] == "b" else None
    _set_env(monkeypatch, dma, blocks)
    cap = blocks if blocks else (5 if sched == "slab5" else (256 if nw8 else 512))
    ntiles = [_cdiv(W, 32) * _cdiv(H, 8 if nw8 else 4) for (H, W) in images]
    expect = [min(t, cap) for t in ntiles]
    per = ops.wgrad_slab_floats(Cin, Cout, K)
    slab = torch.full(((sum(expect) + 2) * per,), NAN, device=dev)
    n, got = 0, []
    for (x, dz, act, H, W) in d["calls"]:
        # the workgroup count is clamped to what the slab holds behind the running offset
        view = slab[:(n + 5) * per] if sched == "slab5" else slab
        k = ops.wgrad_partial_bf16(CV(x.to(dev), 0, Cin), CV(dz.to(dev), 0, Cout), Cout, K, view, n * per,
                                   relu_mask=act.to(dev) if masked else None)
        got.append(k)
        n += k
    name = "%s %s %s %s" % (bname, lid, "+".join("%dx%d" % i for i in images), sched)
    assert got == expect, ("the case fell onto another schedule", name, got, expect)
    gw, gb = d["gw0"].clone().to(dev), d["gb0"].clone().to(dev)
    ops.wgrad_reduce_multi([(slab, n, Cin, Cout, K, gw, gb)], accumulate=True)
    _assert_exact(gw, d["want_w"], name + " grad_w")
    _assert_exact(gb, d["want_b"], name + " grad_b")
    _report(name.replace(" ", "/"), n, "/".join(str(_cdiv(t, e)) for t, e in zip(ntiles, expect)))


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("lid", list(LAYERS))
def test_deferred_partial_and_reduce(backend, lid, sched, monkeypatch):
    """Two weight-gradient calls of one layer appended to one slab region (the second at a non-zero offset, as in training), one
    batched reduction accumulating onto existing integer gradients: exact for every kernel the launch table selects, at every
    tile-loop depth and tile order."""
    _deferred(backend, monkeypatch, lid, IMAGES8 if LAYERS[lid][7] else IMAGES4, sched)


@pytest.mark.parametrize("sched", ["default", "b1"])
@pytest.mark.parametrize("lid", ["c64-64_dma", "c64-64_reg", "c48-48_dma", "c48-48_reg", "c3-48_ld8_dma", "c12-48_ld16_dma"])
def test_deferred_edge_images(backend, lid, sched, monkeypatch):
    """A single pixel, an image of exactly one tile, and one row or column over and under a tile: five calls, one segment."""
    _deferred(backend, monkeypatch, lid, EDGES, sched)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. the reduce kernels on their own: synthetic integer slabs
# ---------------------------------------------------------------------------------------------------------------------------------
# (Cin, Cout, K, slabs, with grad_b): the engine's nine layers, one of them at the 40 -> 40 shape; 65, 130 and 200 slabs take the
# second, third and fourth trip of the `k += 64` loop, 64 and 1 end exactly on / far inside the first
SEGMENTS = [(3, 48, 3, 70, True), (48, 48, 3, 1, True), (48, 3, 1, 130, True), (12, 48, 3, 65, True), (40, 40, 3, 9, True),
            (48, 6, 1, 64, False), (9, 64, 3, 200, True), (64, 64, 3, 3, True), (64, 3, 3, 7, False)]


def _c16(c):
    return (c + 15) // 16 * 16


def _synthetic_segment(g, Cin, Cout, K, nslab, with_b):
    """integer slabs [nslab][tap][ci16][co16] + [co16] with 1000 in the rows / columns beyond the layer (the reduction crops them)
    and two NaN slabs behind the last one (it stops at nslab); -> slabs, initial gradients, float64 sums in grad_w / grad_b layout"""
    _exact_ok(nslab)
    CT, NT, T = _c16(Cin), _c16(Cout), K * K
    w = torch.full((nslab + 2, T, CT, NT), 1000.0)
    w[:, :, :Cin, :Cout] = _ints(g, nslab + 2, T, Cin, Cout)
    b = torch.full((nslab + 2, NT), 1000.0)
    b[:, :Cout] = _ints(g, nslab + 2, Cout)
    slabs = torch.cat([w.reshape(nslab + 2, -1), b], 1)
    slabs[nslab:] = NAN
    sum_w = w[:nslab, :, :Cin, :Cout].double().sum(0).permute(2, 1, 0).reshape(Cout, Cin, K, K)
    sum_b = b[:nslab, :Cout].double().sum(0)
    return slabs.reshape(-1).contiguous(), _ints(g, Cout, Cin, K, K), (_ints(g, Cout) if with_b else None), sum_w, sum_b


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_reduce_multi_segments(backend, accumulate):
    """One wgrad_reduce_multi launch over nine segments of different length (the uniform early return of the short ones), slab
    lists up to 200 long, two segments without a bias gradient."""
    ops, dev, bname = backend
    g = _gen("reduce_multi%d" % accumulate)
    data = [_synthetic_segment(g, *s) for s in SEGMENTS]
    segs, outs = [], []
    for (Cin, Cout, K, nslab, _), (slabs, gw0, gb0, _, _) in zip(SEGMENTS, data):
        gw, gb = gw0.clone().to(dev), (gb0.clone().to(dev) if gb0 is not None else None)
        segs.append((slabs.to(dev), nslab, Cin, Cout, K, gw, gb))
        outs.append((gw, gb))
    ops.wgrad_reduce_multi(segs, accumulate=accumulate)
    for (Cin, Cout, K, nslab, _), (_, gw0, gb0, sum_w, sum_b), (gw, gb) in zip(SEGMENTS, data, outs):
        name = "%s reduce_multi c%d-%d k%d n%d acc%d" % (bname, Cin, Cout, K, nslab, accumulate)
        _assert_exact(gw, gw0.double() + sum_w if accumulate else sum_w, name + " grad_w")
        if gb is not None:
            _assert_exact(gb, gb0.double() + sum_b if accumulate else sum_b, name + " grad_b")
    _report("%s/reduce_multi/acc%d" % (bname, accumulate), "+".join(str(s[3]) for s in SEGMENTS), "-")


def test_reduce_multi_segment_limit(backend):
    """16 segments (ZT_MAXSEG) reduce in one launch; 17 are refused before anything is launched."""
    ops, dev, bname = backend
    g = _gen("reduce_limit")
    Cin, Cout, K, nslab = 48, 3, 1, 2
    data = [_synthetic_segment(g, Cin, Cout, K, nslab, True) for _ in range(17)]
    segs = [(d[0].to(dev), nslab, Cin, Cout, K, d[1].clone().to(dev), d[2].clone().to(dev)) for d in data]
    with pytest.raises(RuntimeError, match="zt_wgrad_reduce_multi_f32 failed"):
        ops.wgrad_reduce_multi(segs, accumulate=True)
    for s, d in zip(segs, data):
        _assert_exact(s[5], d[1].double(), "%s refused launch left grad_w alone" % bname)
        _assert_exact(s[6], d[2].double(), "%s refused launch left grad_b alone" % bname)
    ops.wgrad_reduce_multi(segs[:16], accumulate=True)
    for s, d in zip(segs[:16], data):
        _assert_exact(s[5], d[1].double() + d[3], "%s 16 segments grad_w" % bname)
        _assert_exact(s[6], d[2].double() + d[4], "%s 16 segments grad_b" % bname)
    _assert_exact(segs[16][5], data[16][1].double(), "%s segment 17 untouched" % bname)
    _report("%s/reduce_multi/16_segments" % bname, "16x%d" % nslab, "-")


def test_reduce_single_segment_past_64_slabs(backend, monkeypatch):
    """wgrad_reduce_kernel behind conv2d_wgrad_bf16: 49 x 129 is 13 x 5 = 65 tiles of 4 x 32, the smallest tile grid with interior
    and ragged tiles that takes the second trip of its `k += 64` loop; overwrite, then accumulate."""
    ops, dev, bname = backend
    CV = _cv()
    _set_env(monkeypatch)
    lid, H, W = "c40-40_ld40", 49, 129
    Cin, ldx, Cout, lddz, K = LAYERS[lid][:5]
    key = ("single", lid, H, W)
    if key not in _CACHE:
        g = _gen(repr(key))
        _exact_ok(H * W, 2)
        x, dz = _ints(g, 1, Cin, H, W), _ints(g, 1, Cout, H, W)
        _CACHE[key] = (_nhwc(x, ldx), _nhwc(dz, lddz), _ints(g, Cout, Cin, K, K), _ints(g, Cout)) + _wgrad_ref(x, dz, K)
    x, dz, gw0, gb0, ref_w, ref_b = _CACHE[key]
    ntiles = _cdiv(W, 32) * _cdiv(H, 4)
    assert ntiles == 65
    slab = torch.full(((ntiles + 2) * ops.wgrad_slab_floats(Cin, Cout, K),), NAN, device=dev)
    gw, gb = gw0.clone().to(dev), gb0.clone().to(dev)
    xv, dzv = CV(x.to(dev), 0, Cin), CV(dz.to(dev), 0, Cout)
    for acc, mult in ((False, 1), (True, 2)):
        ops.conv2d_wgrad_bf16(xv, dzv, Cout, K, K, gw, accumulate=acc, slab=slab, grad_b=gb)
        _assert_exact(gw, mult * ref_w, "%s single reduce acc%d grad_w" % (bname, acc))
        _assert_exact(gb, mult * ref_b, "%s single reduce acc%d grad_b" % (bname, acc))
    assert bool(torch.isnan(slab[ntiles * ops.wgrad_slab_floats(Cin, Cout, K):]).all())      # 65 slabs, no more
    _report("%s/reduce_single/%s/%dx%d" % (bname, lid, H, W), ntiles, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. fp32 wgrad_mfma_f32_kernel: grid-stride tile loop, bsum carried across tiles, the slab_bytes clamp
# ---------------------------------------------------------------------------------------------------------------------------------
F32_CASES = [(3, 48, 3, 4), (48, 48, 3, 48), (48, 3, 1, 48), (9, 64, 3, 12), (64, 64, 3, 64), (64, 3, 3, 64), (12, 48, 3, 12), (48, 6, 1, 48)]


@pytest.mark.parametrize("cap", [None, 1, 2, 5], ids=lambda c: "cap%s" % c)
@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: "c%d-%d_k%d" % c[:3])
def test_wgrad_f32_depths(backend, case, cap):
    """13 x 37 is 4 x 3 = 12 tiles of 4 x 16; a slab of cap workgroups gives 12, 6 and 2-3 tiles per workgroup (None: one each)."""
    ops, dev, bname = backend
    CV = _cv()
    Cin, Cout, K, ldx = case
    H, W = 13, 37
    key = ("f32", case)
    if key not in _CACHE:
        g = _gen(repr(key))
        _exact_ok(H * W, 2)
        x, dz = _ints(g, 1, Cin, H, W), _ints(g, 1, Cout, H, W)
        _CACHE[key] = (_nhwc(x, ldx, dtype=torch.float32), _nhwc(dz, (Cout + 3) // 4 * 4, dtype=torch.float32),
                       _ints(g, Cout, Cin, K, K), _ints(g, Cout)) + _wgrad_ref(x, dz, K)
    x, dz, gw0, gb0, ref_w, ref_b = _CACHE[key]
    ntiles = _cdiv(W, 16) * _cdiv(H, 4)
    nblk = ntiles if cap is None else cap
    per = ops.wgrad_slab_floats(Cin, Cout, K)
    slab = torch.full(((ntiles + 4 if cap is None else cap) * per,), NAN, device=dev)
    gw, gb = gw0.clone().to(dev), gb0.clone().to(dev)
    xv, dzv = CV(x.to(dev), 0, Cin), CV(dz.to(dev), 0, Cout)
    name = "%s f32 c%d-%d k%d %dx%d cap=%s" % (bname, Cin, Cout, K, H, W, cap)
    ops.conv2d_wgrad(xv, dzv, Cout, K, K, gw, accumulate=True, slab=slab, grad_b=gb)
    _assert_exact(gw, gw0.double() + ref_w, name + " accumulate grad_w")
    _assert_exact(gb, gb0.double() + ref_b, name + " accumulate grad_b")
    ops.conv2d_wgrad(xv, dzv, Cout, K, K, gw, accumulate=False, slab=slab, grad_b=gb)
    _assert_exact(gw, ref_w, name + " overwrite grad_w")
    _assert_exact(gb, ref_b, name + " overwrite grad_b")
    if cap is None:
        assert bool(torch.isnan(slab[ntiles * per:]).all()) and not bool(torch.isnan(slab[:ntiles * per]).any())
    _report(name.replace(" ", "/"), nblk, "%d-%d" % (ntiles // nblk, _cdiv(ntiles, nblk)))


# ---------------------------------------------------------------------------------------------------------------------------------
# D. thin 1x1 backward appended to a segment that a wgrad_partial_bf16 call of the same layer shape started
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cdr", [3, 6])
def test_thin1x1_bwd_into_shared_segment(backend, Cdr, monkeypatch):
    """48 -> Cdr 1x1 layer: a generic partial call on 9 x 41, then thin1x1_bwd_bf16 on 27 x 101 at the offset behind it, one reduce.
    Weight and bias gradients are exact.  dz2 = (w3^T dr) * [a2 > 0 ? 1 : 0.2]: w3 in [-2, 2] makes w3^T dr an integer below 2^8,
    bf16-exact, so it must come out exactly where the factor is 1; the kernel multiplies by 0.2f in fp32 and rounds the product to
    bf16 (zt_conv_thin.hip), one rounding stage: |got - r| <= 2^-8 |r| (half a bf16 unit in the last place) + 2 * 2^-23 |r| (0.2f
    and the fp32 product, 2^-24 each, with a factor 2 to spare), r = 0.2 w3^T dr in float64."""
    ops, dev, bname = backend
    CV = _cv()
    _set_env(monkeypatch)
    (H0, W0), (H, W) = (9, 41), (27, 101)
    key = ("thin1x1", Cdr)
    if key not in _CACHE:
        g = _gen(repr(key))
        _exact_ok(H0 * W0 + H * W)
        a0, d0, a2, dr = _ints(g, 1, 48, H0, W0), _ints(g, 1, Cdr, H0, W0), _ints(g, 1, 48, H, W), _ints(g, 1, Cdr, H, W)
        w3 = _ints(g, Cdr, 48, 1, 1, lo=-2, hi=2)
        v = torch.einsum("oi,nohw->nihw", w3[:, :, 0, 0].double(), dr.double())
        assert float(v.abs().max()) < 2 ** 8
        ref_w = torch.einsum("nohw,nihw->oi", d0.double(), a0.double()) + torch.einsum("nohw,nihw->oi", dr.double(), a2.double())
        _CACHE[key] = dict(a0=_nhwc(a0, 48), d0=_nhwc(d0, 8), a2=_nhwc(a2, 56), dr=_nhwc(dr, 8), w3=w3, v=v, pos=a2 > 0,
                           gw0=_ints(g, Cdr, 48, 1, 1), gb0=_ints(g, Cdr), ref_w=ref_w.reshape(Cdr, 48, 1, 1),
                           ref_b=d0.double().sum(dim=(0, 2, 3)) + dr.double().sum(dim=(0, 2, 3)))
    d = _CACHE[key]
    per = ops.wgrad_slab_floats(48, Cdr, 1)
    n0_expect, n1_expect = _cdiv(W0, 32) * _cdiv(H0, 4), _cdiv(_cdiv(H * W, 4), 42)
    slab = torch.full(((n0_expect + n1_expect + 2) * per,), NAN, device=dev)
    n0 = ops.wgrad_partial_bf16(CV(d["a0"].to(dev), 0, 48), CV(d["d0"].to(dev), 0, Cdr), Cdr, 1, slab, 0)
    wT = ops.repack_weight_bf16(d["w3"].to(dev), transpose_flip=True)
    dz2, n1 = ops.thin1x1_bwd_bf16(d["dr"].to(dev), Cdr, wT, d["a2"].to(dev), slab, n0 * per)
    assert (n0, n1) == (n0_expect, n1_expect)
    gw, gb = d["gw0"].clone().to(dev), d["gb0"].clone().to(dev)
    ops.wgrad_reduce_multi([(slab, n0 + n1, 48, Cdr, 1, gw, gb)], accumulate=True)
    name = "%s thin1x1_bwd c48-%d %dx%d+%dx%d" % (bname, Cdr, H0, W0, H, W)
    _assert_exact(gw, d["gw0"].double() + d["ref_w"], name + " grad_w")
    _assert_exact(gb, d["gb0"].double() + d["ref_b"], name + " grad_b")
    got = dz2.cpu().double().permute(0, 3, 1, 2)
    v, pos = d["v"], d["pos"]
    _assert_exact(torch.where(pos, got, v), v, name + " dz2 where a2 > 0")
    r = 0.2 * v
    err, bound = (got - r).abs()[~pos], ((U8 + 2 * U23) * r.abs())[~pos]
    print("WGRADEXACT %s dz2 leaky pixels worst_err_over_bound=%.3g" % (name.replace(" ", "/"), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), (name, float((err - bound).max()))
    _report(name.replace(" ", "/"), "%d+%d" % (n0, n1), "1/%d" % _cdiv(_cdiv(H * W, 4), 42 * n1))


# ---------------------------------------------------------------------------------------------------------------------------------
# E. repack_weights_bf16_multi
# ---------------------------------------------------------------------------------------------------------------------------------
REPACK_SHAPES = [(48, 3, 3), (48, 48, 3), (3, 48, 1), (64, 64, 3), (64, 12, 3), (6, 48, 1), (126, 256, 3)]      # Cout, Cin, K


def test_repack_multi_equals_single(backend):
    """Fourteen entries (each shape plain and transposed / flipped; 126 x 256 x 3 passes the 64-block grid cap and runs the
    grid-stride loop) in one launch: equal to repack_weight_bf16 entry by entry from identical output contents, equal to a torch
    permutation of w.bfloat16() in the written region, and the padding rows / columns keep what they held -- both forms leave
    zeroing them to the caller."""
    ops, dev, bname = backend
    g = _gen("repack")
    SENT = -512.0
    entries, singles, wants = [], [], []
    for (Cout, Cin, K) in REPACK_SHAPES:
        w = torch.randn(Cout, Cin, K, K, generator=g)
        wd = w.to(dev)
        for flip in (False, True):
            n_out, n_in = (Cin, Cout) if flip else (Cout, Cin)
            shape = (K * K, _c16(n_out), (n_in + 7) // 8 * 8)
            out = torch.full(shape, SENT, dtype=torch.bfloat16, device=dev)
            one = torch.full(shape, SENT, dtype=torch.bfloat16, device=dev)
            ops.repack_weight_bf16(wd, transpose_flip=flip, out=one)
            want = torch.full(shape, SENT, dtype=torch.bfloat16)
            wb = w.bfloat16()
            want[:, :n_out, :n_in] = (wb.flip(2, 3).permute(2, 3, 1, 0) if flip else wb.permute(2, 3, 0, 1)).reshape(K * K, n_out, n_in)
            entries.append((wd, out, flip))
            singles.append(one)
            wants.append(want)
    assert len(entries) == 14
    ops.repack_weights_bf16_multi(entries)
    for (wd, out, flip), one, want in zip(entries, singles, wants):
        name = "%s repack %s flip=%d" % (bname, tuple(wd.shape), flip)
        assert torch.equal(out.cpu(), one.cpu()), name + ": multi != single"
        assert torch.equal(out.cpu(), want), name + ": != torch permutation / padding overwritten"
    _report("%s/repack_multi" % bname, len(entries), "-")
