"""The tile loops of the three persistent convolution kernels -- conv_rs_bf16_kernel (zt_conv_rs.hip), conv_ws_bf16_kernel
(zt_conv_ws.hip), denoise_fused_bf16_kernel (zt_denoise.hip) -- and the grid-stride loop of thin1x1_bwd_bf16_kernel, at every
depth (tiles per workgroup) that the hand-over between consecutive tiles distinguishes.  ZT_CONV_BLOCKS caps the workgroups of a
launch, so a 15-tile image runs at depth 1, 2, 5 and 15.  Every case asserts

 (a) schedule independence: a pixel's arithmetic does not depend on which workgroup computes its tile, so the capped launch
     equals the default launch (one tile per workgroup at these sizes) bit for bit;
 (b) every element against F.conv2d in float64 on the bf16-rounded operands, within a bound derived from the number formats:

        |got - ref| <= sum over the kernel's bf16 rounding stages of 2^-8 |value rounded| + f,   f = (n + 2) 2^-23 A,

     n = Cin KH KW, A = conv(|x|, |w|) + |b| in float64.  2^-8 |v| is half a bf16 unit in the last place of v (8 significand
     bits); the value a stage rounds is known to within the error of the stages before it, which the bound carries along.  f
     bounds the fp32 accumulation of n products, the bias and the activation in ANY order (n + 2 roundings of 2^-24 A each) with
     a factor 2 to spare, which also covers the one further fp32 operation of a fused epilogue.  Nothing in it is measured.
     ReLU, LeakyReLU, the clamped sigmoid and the 0 / 0.2 / 1 masks do not enlarge an error (Lipschitz constant <= 1).

The rounding stages, read from the kernels: rs with 48 couts applies the epilogue to the fp32 accumulators (one stage: the stored
value); rs with 64 couts and ws stage act(conv) as bf16 and apply the epilogue to the staged value (epi 3: staged value and sum;
epi 1: staged value and, where the mask factor is 0.2, the product; a factor 0 or 1 is exact); fp32 outputs have none.
The aux operand is bf16-exact, so the masks are deterministic.  Worst err / bound per case is printed (CONVPERSIST lines)."""
import math

import pytest
import torch
import torch.nn.functional as F
from importlib import import_module

U8, U23, U24 = 2.0 ** -8, 2.0 ** -23, 2.0 ** -24


def _report(what, name, **figs):
    print("CONVPERSIST %s [%s] %s" % (what, name, " ".join("%s=%.3g" % kv for kv in figs.items())))


def _bf(t):
    return t.bfloat16().float()


def _nhwc_bf16(t, ld, fill=0.0):
    """NCHW -> bf16 NHWC with ld channel slots; the padding slots hold `fill`"""
    n = t.permute(0, 2, 3, 1)
    out = torch.full((*n.shape[:3], ld), fill)
    out[..., :n.shape[-1]] = n
    return out.bfloat16().contiguous()


def _nchw64(y, C):
    return y.detach().cpu()[..., :C].double().permute(0, 3, 1, 2)


def _set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("ZT_CONV_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("ZT_CONV_BLOCKS", str(cap))


ACTS = {None: lambda t: t, "relu": torch.relu, "lrelu": lambda t: F.leaky_relu(t, 0.2),
        "sigmoid_clamp": lambda t: torch.clamp(torch.sigmoid(t), 1e-4, 1)}

_CACHE = {}


def _conv_case(Cin, Cout, K, act, epi, H, W, rounding):
    """Operands (bf16-exact, fp32 NCHW), float64 reference and elementwise bound of one layer.  rounding: "fused" (one bf16 stage,
    epilogue on the accumulators), "staged" (act(conv) rounded to bf16, then the epilogue), "fp32" (no bf16 stage).  Built once
    per case and shared by both back-ends; never modified."""
    key = (Cin, Cout, K, act, epi, H, W, rounding)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + epi + H)
    x = _bf(torch.randn(1, Cin, H, W, generator=g))
    w = _bf(torch.randn(Cout, Cin, K, K, generator=g) / (Cin * K * K) ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.1
    aux = _bf(torch.randn(1, Cout, H, W, generator=g))
    xd, wd, bd, ad = x.double(), w.double(), b.double(), aux.double()
    c = F.conv2d(xd, wd, bd, padding=K // 2)
    A = F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=K // 2)
    f = (Cin * K * K + 2) * U23 * A
    v = ACTS[act](c)
    m = None if epi in (0, 3) else torch.where(ad > 0, 1.0, 0.2 if epi == 1 else 0.0).double()
    ref = v if epi == 0 else (v + ad if epi == 3 else v * m)
    if rounding == "fp32":
        bound = f
    elif rounding == "fused" or epi == 0:
        bound = U8 * (ref.abs() + f) + f
    else:
        e1 = U8 * (v.abs() + f) + f                                   # the staged act(conv)
        if epi == 3:
            bound = e1 + U8 * (ref.abs() + e1)
        else:
            bound = m * e1 + torch.where((m > 0) & (m < 1), U8 * (ref.abs() + m * e1), torch.zeros_like(ref))
    _CACHE[key] = dict(x=x, w=w, b=b, aux=aux, ref=ref, bound=bound)
    return _CACHE[key]


def _check(got, d, what, name):
    err = (got - d["ref"]).abs()
    ratio = float((err / d["bound"].clamp_min(1e-300)).max())
    _report(what, name, worst_err_over_bound=ratio, max_err=float(err.max()), max_ref=float(d["ref"].abs().max()))
    assert bool((err <= d["bound"]).all()), (what, name, ratio)


def _launch(ops, dev, d, Cin, Cout, K, act, epi, variant, planar=False):
    CV = import_module("zero-tig_amd.ops").CV
    ld = (Cin + 7) // 8 * 8
    xdev = _nhwc_bf16(d["x"], ld, fill=1000.0).to(dev)               # padding slots of a pixel are not the layer's: garbage
    y = ops.conv2d_bf16(CV(xdev, 0, Cin), ops.repack_weight_bf16(d["w"].to(dev)), d["b"].to(dev), Cout, K, K, (K // 2, K // 2), act,
                        aux=_nhwc_bf16(d["aux"], Cout).to(dev) if epi else None, epi=epi, variant=variant, out_planar=planar)
    return y.cpu()


def _depth_case(backend, monkeypatch, family, layer, H, W, caps, planar=False):
    ops, dev, bname = backend
    Cin, Cout, K, act, epi = layer
    variant = 3 if family == "rs" else 1
    rounding = "fp32" if planar else ("fused" if family == "rs" and Cout == 48 else "staged")
    d = _conv_case(Cin, Cout, K, act, epi, H, W, rounding)
    base = None
    for cap in caps:
        _set_cap(monkeypatch, cap)
        y = _launch(ops, dev, d, Cin, Cout, K, act, epi, variant, planar)
        name = "%s %s c%d-%d k%d %s epi%d %dx%d cap=%s" % (bname, family, Cin, Cout, K, act, epi, H, W, cap)
        if base is None:
            base = y
            _check(y.double() if planar else _nchw64(y, Cout), d, "fp64", name)
        else:
            assert torch.equal(y, base), ("schedule dependence", name)


# ------------------------------------------------------------------------------------------------------------ rs
RS_LAYERS = [(64, 64, 3, "relu", 0), (64, 64, 3, "relu", 3), (48, 48, 3, "lrelu", 1), (9, 64, 3, "relu", 0), (12, 48, 3, "lrelu", 0),
             (3, 48, 3, "lrelu", 2), (56, 64, 3, "relu", 0), (40, 48, 3, "lrelu", 0)]
_lid = lambda c: "c%d-%d_k%d_epi%d" % (c[0], c[1], c[2], c[4])


@pytest.mark.parametrize("hw", [(18, 70), (22, 100)], ids=["18x70", "22x100"])
@pytest.mark.parametrize("layer", RS_LAYERS, ids=_lid)
def test_rs_depths(backend, layer, hw, monkeypatch):
    """conv_rs_bf16_kernel, tiles of 4 x 32.  18 x 70: 5 x 3 tiles, the last band has one tile row, the last row 2 px, the last
    column 6 px.  22 x 100: 6 x 4 = 24 tiles, the second band has two tile rows.  Caps 16 / 8: the XCD permutation with G / 8 = 2
    and 1 and mixed depths (on 15 tiles, cap 16 is the default grid); 3: plain order, depth >= 5, both halo buffers recycled and the
    hidden aux loads waited for by count on every tile with a successor; 1: one workgroup walks the image.  Every instantiation
    that rs_ok admits, Cin 56 and 40 included."""
    _depth_case(backend, monkeypatch, "rs", layer, hw[0], hw[1], (None, 16, 8, 3, 1))


@pytest.mark.parametrize("layer", [(64, 64, 3, "relu", 0), (64, 64, 3, "relu", 3), (48, 48, 3, "lrelu", 1), (9, 64, 3, "relu", 0)], ids=_lid)
def test_rs_beyond_tile_table(backend, layer, monkeypatch):
    """258 x 100: 65 x 4 = 260 tiles on ONE workgroup: depth 260 exceeds the 256-entry LDS table of tile coordinates, so tiles
    256..259 (the last band: one tile row of 2 px) take the recomputed tile_calc path that an 8K frame takes on the default grid."""
    _depth_case(backend, monkeypatch, "rs", layer, 258, 100, (None, 1))


def test_rs_views(backend, monkeypatch):
    """x, aux and out are channel-offset views (offsets a multiple of 8 elements) into wider buffers filled with a bf16-exact
    sentinel; 64 -> 64 with the residual epilogue, 18 x 70, three workgroups.  Everything outside the output window stays."""
    ops, dev, bname = backend
    CV = import_module("zero-tig_amd.ops").CV
    H, W = 18, 70
    d = _conv_case(64, 64, 3, "relu", 3, H, W, "staged")
    xb = torch.full((1, H, W, 80), 1000.0)
    xb[..., 8:72] = d["x"].permute(0, 2, 3, 1)
    ab = torch.full((1, H, W, 72), -1000.0)
    ab[..., 8:72] = d["aux"].permute(0, 2, 3, 1)
    wdev, bdev = ops.repack_weight_bf16(d["w"].to(dev)), d["b"].to(dev)
    xdev, adev = xb.bfloat16().to(dev), ab.bfloat16().to(dev)
    outs = []
    for cap in (None, 3):
        _set_cap(monkeypatch, cap)
        out = torch.full((1, H, W, 88), 3.0, dtype=torch.bfloat16, device=dev)
        ops.conv2d_bf16(CV(xdev, 8, 64), wdev, bdev, 64, 3, 3, (1, 1), "relu", out=CV(out, 16, 64), aux=CV(adev, 8, 64), epi=3, variant=3)
        o = out.cpu()
        assert bool((o[..., :16] == 3.0).all()) and bool((o[..., 80:] == 3.0).all()), "wrote outside the output window"
        outs.append(o[..., 16:80].contiguous())
    assert torch.equal(outs[0], outs[1]), "schedule dependence"
    _check(_nchw64(outs[1], 64), d, "fp64", "%s rs views c64-64 epi3 18x70 cap=3" % bname)
    # the same operands as plain tensors: a view changes addresses only
    _set_cap(monkeypatch, 3)
    assert torch.equal(_launch(ops, dev, d, 64, 64, 3, "relu", 3, 3), outs[1])


def _sum_check(got, terms, what, name):
    """fp32 sums of n_px terms per channel, in any order, against the float64 sum of the same terms"""
    n_px = terms.shape[0]
    ref, bound = terms.sum(0), n_px * U24 * terms.abs().sum(0)
    err = (got - ref).abs()
    _report(what, name, worst_err_over_bound=float((err / bound.clamp_min(1e-300)).max()), max_err=float(err.max()))
    assert bool((err <= bound).all()), (what, name)


STAT_CAPS = (None, 8, 3, 1)


def test_rs_fused_bn_stats_depths(backend, monkeypatch):
    """conv3x3_bn_stats_bf16 on the fused kernel (forward statistics accumulated in stat_s across a workgroup's tiles), 18 x 70 =
    15 tiles on 15 / 8 / 3 / 1 workgroups: y bit-equal across caps and within the fp64 bound; rows of `part` at and beyond the grid
    size exactly 0 and every row below it written; the sums are those of the STORED values, fp32 in some order."""
    ops, dev, bname = backend
    CV = import_module("zero-tig_amd.ops").CV
    monkeypatch.setenv("ZT_STATS_FUSE_MIN_TILES", "1")
    H, W = 18, 70
    d = _conv_case(64, 64, 3, None, 0, H, W, "staged")
    xdev, wdev, bdev = _nhwc_bf16(d["x"], 64).to(dev), ops.repack_weight_bf16(d["w"].to(dev)), d["b"].to(dev)
    base = None
    for cap in STAT_CAPS:
        _set_cap(monkeypatch, cap)
        y, part = ops.conv3x3_bn_stats_bf16(CV(xdev, 0, 64), wdev, bdev, 64)
        y, part = y.cpu(), part.cpu()[0]
        name = "%s bn_stats 18x70 cap=%s" % (bname, cap)
        grid = 15 if cap is None else cap
        assert bool((part[grid:] == 0).all()), ("rows beyond the grid", name)
        assert bool((part[:grid, 1].sum(dim=1) > 0).all()), ("a workgroup wrote no statistics", name)
        if base is None:
            base = y
            _check(_nchw64(y, 64), d, "fp64", name)
        else:
            assert torch.equal(y, base), ("schedule dependence", name)
        stored = y.double().view(H * W, 64)
        s = part.double().sum(dim=0)
        _sum_check(s[0], stored, "sum", name)
        _sum_check(s[1], stored * stored, "sumsq", name)


def test_rs_fused_bn_bwd_sums_depths(backend, monkeypatch):
    """conv3x3_dgrad_bn_sums_bf16 (data gradient + residual + the BatchNorm-backward sums of the block below) at the same depths.
    scale / shift are bf16-exact, so z * scale is exact in fp32 and the sign of z * scale + shift -- the ReLU mask -- does not
    depend on rounding or contraction."""
    ops, dev, bname = backend
    H, W = 18, 70
    d = _conv_case(64, 64, 3, None, 3, H, W, "staged")               # x plays dz, w the transposed-flipped operator, aux the residual
    g = torch.Generator().manual_seed(77)
    z = _bf(torch.randn(1, 64, H, W, generator=g) * 2.0)
    scale, shift = _bf(torch.rand(64, generator=g) + 0.5), _bf(torch.randn(64, generator=g) * 0.3)
    mean = _bf(torch.randn(64, generator=g) * 0.3)
    dzd, resd, zd = (_nhwc_bf16(t, 64).to(dev) for t in (d["x"], d["aux"], z))
    wdev = ops.repack_weight_bf16(d["w"].to(dev))
    zf = z.double().permute(0, 2, 3, 1).reshape(H * W, 64)
    mask = zf * scale.double() + shift.double() > 0
    base = None
    for cap in STAT_CAPS:
        _set_cap(monkeypatch, cap)
        df, part = ops.conv3x3_dgrad_bn_sums_bf16(dzd, wdev, resd, zd, scale.to(dev), shift.to(dev), mean.to(dev))
        df, part = df.cpu(), part.cpu()
        name = "%s bn_bwd_sums 18x70 cap=%s" % (bname, cap)
        grid = 15 if cap is None else cap
        assert bool((part[grid:] == 0).all()), ("rows beyond the grid", name)
        assert bool((part[:grid].abs().sum(dim=(1, 2)) > 0).all()), ("a workgroup wrote no sums", name)
        if base is None:
            base = df
            # no bias in the data gradient: the operand's bias is not passed
            ref = F.conv2d(d["x"].double(), d["w"].double(), None, padding=1)
            A = F.conv2d(d["x"].double().abs(), d["w"].double().abs(), None, padding=1)
            f = (576 + 2) * U23 * A
            e1 = U8 * (ref.abs() + f) + f
            tot = ref + d["aux"].double()
            _check(_nchw64(df, 64), dict(ref=tot, bound=e1 + U8 * (tot.abs() + e1)), "fp64", name)
        else:
            assert torch.equal(df, base), ("schedule dependence", name)
        gm = torch.where(mask, df.double().view(H * W, 64), torch.zeros(H * W, 64, dtype=torch.float64))
        s = part.double().sum(dim=0)
        _sum_check(s[0], gm, "sum_g", name)
        _sum_check(s[1], gm * (zf - mean.double()), "sum_g_zc", name)


# ------------------------------------------------------------------------------------------------------------ ws
WS_LAYERS = [(64, 3, 3, "sigmoid_clamp", 0, True), (48, 48, 3, "lrelu", 1, False), (64, 64, 3, "relu", 3, False), (12, 48, 3, None, 0, False),
             (48, 6, 1, None, 0, True)]


@pytest.mark.parametrize("layer", WS_LAYERS, ids=lambda c: _lid(c) + ("_planar" if c[5] else ""))
def test_ws_depths(backend, layer, monkeypatch):
    """conv_ws_bf16_kernel, tiles of 8 x 32, 19 x 70 = 3 x 3 tiles on 9 / 5 / 2 / 1 workgroups (depth 1, 2, 5, 9): the register
    prefetch of the next halo and the output staging that aliases the halo buffer.  The layers are those that take ws on the product
    path -- the planar fp32 output layers -- and one of each remaining code path: the bf16 epilogues on the staged tile (epi 1, 3),
    two cout groups in grid.y (64 -> 64), the one-chunk instantiation (Cin 12)."""
    _depth_case(backend, monkeypatch, "ws", layer[:5], 19, 70, (None, 5, 2, 1), planar=layer[5])


# ------------------------------------------------------------------------------------------------------------ denoise
def _denoise_case(kind, H, W):
    key = ("dn", kind, H, W)
    if key in _CACHE:
        return _CACHE[key]
    gen = torch.Generator().manual_seed(31 if kind == "D1" else 32)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    ng, cout = (1, 3) if kind == "D1" else (4, 6)
    cin = 3 * ng
    w1, b1 = rnd(48, cin, 3, 3) * (0.6 / math.sqrt(9 * cin)), rnd(48) * 0.1
    w2, b2 = rnd(48, 48, 3, 3) * (1.0 / math.sqrt(9 * 48)), rnd(48) * 0.1
    w3, b3 = rnd(cout, 48, 1, 1) * (0.5 / math.sqrt(48)), rnd(cout) * 0.05
    planes = [torch.rand(1, 3, H, W, generator=gen) for _ in range(ng)]
    refs = [planes[0]] if kind == "D1" else [planes[2], planes[3]]

    def chain(dt):
        """the kernel's chain in precision dt: bf16 operands, a1 and a2 rounded to bf16 where the kernel rounds them"""
        c = lambda t: t.to(dt)
        rb = lambda t: t.bfloat16().to(dt)
        a1 = rb(F.leaky_relu(F.conv2d(rb(torch.cat(planes, 1)), rb(w1), c(b1), padding=1), 0.2))
        a2 = rb(F.leaky_relu(F.conv2d(a1, rb(w2), c(b2), padding=1), 0.2))
        r = F.conv2d(a2, rb(w3), c(b3))
        return r, (c(torch.cat(refs, 1)) - r).clamp(1e-4, 1)
    r64, o64 = chain(torch.float64)
    r32, o32 = chain(torch.float32)
    E = {"res": float((r32.double() - r64).abs().max()), "out": float((o32.double() - o64).abs().max())}
    _CACHE[key] = dict(planes=planes, refs=refs, w=(w1, w2, w3), b=(b1, b2, b3), cout=cout, r64=r64, o64=o64, E=E)
    return _CACHE[key]


@pytest.mark.parametrize("kind", ["D1", "D2"])
def test_denoise_depths(backend, kind, monkeypatch):
    """denoise_fused_bf16_kernel, tiles of 8 x 32, 19 x 70 = 9 tiles on 9 / 5 / 2 / 1 workgroups: xs and a1s are re-used by a
    workgroup's next tile.  `out` and `res` bit-equal across caps; every element against the float64 chain that rounds a1 and a2 to
    bf16 where the kernel does.  A worst-case propagation through three layers gives a useless ~0.1 max|r|, so the tolerance is
    4 x E, E = the max-abs error of the same chain in torch fp32 on the CPU against that float64 chain, measured here per case; the
    factor stands for MFMA's blocked summation order and for one-ulp flips of a1 / a2.  (This replaces nothing: the rel-L2 gate of
    test_infer.py stays; a few wrong pixels at one tile seam pass that one and fail this one.)"""
    ops, dev, bname = backend
    H, W = 19, 70
    d = _denoise_case(kind, H, W)
    dd = lambda t: t.to(dev).contiguous()
    srcs = [dd(p) for p in d["planes"]]
    refs = [srcs[0]] if kind == "D1" else [srcs[2], srcs[3]]
    wd = [ops.repack_weight_bf16(dd(w)) for w in d["w"]]
    bd = [dd(b) for b in d["b"]]
    base = None
    for cap in (None, 5, 2, 1):
        _set_cap(monkeypatch, cap)
        o, r = ops.denoise_fused_bf16(srcs, refs, wd[0], bd[0], wd[1], bd[1], wd[2], bd[2], d["cout"], want_res=True)
        o, r = o.cpu(), r.cpu()
        if base is None:
            base = (o, r)
        else:
            assert torch.equal(o, base[0]) and torch.equal(r, base[1]), ("schedule dependence", kind, cap)
    err_r = float((base[1].double() - d["r64"]).abs().max())
    err_o = float((base[0].double() - d["o64"]).abs().max())
    _report("denoise", "%s %s 19x70" % (bname, kind), E_res=d["E"]["res"], err_res=err_r, E_out=d["E"]["out"], err_out=err_o,
            max_res=float(d["r64"].abs().max()))
    assert err_r <= 4 * d["E"]["res"], (kind, "res", err_r, d["E"]["res"])
    assert err_o <= 4 * d["E"]["out"], (kind, "out", err_o, d["E"]["out"])


# ------------------------------------------------------------------------------------------------------------ thin 1x1 backward
@pytest.mark.parametrize("Cdr", [6, 3])
def test_thin1x1_bwd_grid_stride(backend, Cdr):
    """thin1x1_bwd_bf16_kernel grid-strides when it has fewer slabs than groups of 42 x 4 pixels: the launcher shrinks the grid to
    the slab tensor it is given, so tensors of exactly 1, 2 and 3 slabs run 27 x 101 (17 groups) at depth 17, 9 and 6.  dz bit-equal
    to the full launch and within one bf16 rounding of float64; the reduced weight / bias gradients against float64 sums of the
    exact bf16 x bf16 products within n_px 2^-24 sum|term| (the operands are bf16-exact: no input-rounding term)."""
    ops, dev, bname = backend
    H, W = 27, 101
    n_px = H * W
    g = torch.Generator().manual_seed(400 + Cdr)
    a2 = _bf(torch.randn(1, 48, H, W, generator=g))
    dr = _bf(torch.randn(1, Cdr, H, W, generator=g))
    w3 = _bf(torch.randn(Cdr, 48, 1, 1, generator=g) * 0.2)
    wT = ops.repack_weight_bf16(w3.to(dev), transpose_flip=True)
    a2d, drd = _nhwc_bf16(a2, 48).to(dev), _nhwc_bf16(dr, 8, fill=float("nan")).to(dev)
    per = ops.wgrad_slab_floats(48, Cdr, 1)
    A2, DR = a2.double().permute(0, 2, 3, 1).reshape(n_px, 48), dr.double().permute(0, 2, 3, 1).reshape(n_px, Cdr)
    Wm = w3.double().view(Cdr, 48)
    m = torch.where(A2 > 0, 1.0, 0.2).double()
    v, f = (DR @ Wm) * m, (8 + 2) * U23 * (DR.abs() @ Wm.abs())
    dz_ref = dict(ref=v, bound=U8 * (v.abs() + f) + f)
    base = None
    for nslab in (600, 1, 2, 3):
        slab = torch.full((nslab * per,), float("nan"), device=dev)
        dz, n = ops.thin1x1_bwd_bf16(drd, Cdr, wT, a2d, slab, 0)
        name = "%s thin1x1_bwd c%d 27x101 slabs=%d" % (bname, Cdr, n)
        assert n == (17 if nslab == 600 else nslab)
        dz = dz.cpu()
        if base is None:
            base = dz
            _check(dz.double().view(n_px, 48), dz_ref, "fp64", name)
        else:
            assert torch.equal(dz, base), ("schedule dependence", name)
        gw, gb = torch.zeros(Cdr, 48, 1, 1, device=dev), torch.zeros(Cdr, device=dev)
        ops.wgrad_reduce_multi([(slab, n, 48, Cdr, 1, gw, gb)], accumulate=False)
        terms = DR.view(n_px, Cdr, 1) * A2.view(n_px, 1, 48)
        _sum_check(gw.cpu().double().view(Cdr, 48), terms, "grad_w", name)
        _sum_check(gb.cpu().double(), DR, "grad_b", name)
