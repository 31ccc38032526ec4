"""The normalisation family (zt_norm.hip), one entry point at a time against plain torch in fp64.

Covers what test_kernels.py's three norm tests (torch fp32 references, dense buffers, C in {64, 96, 128}) do not reach: the
statistics kernels at awkward channel counts (Q = C / 4 = 1, 2, 3; the C > 256 pass loop of the finalize kernel and of the
one-launch tail), ragged and empty pixel ranges, the auto nblk = 256 of every map of 128 x 128 or more, channel-sliced views
(ld != C) on the 16-byte and on the 8-byte path, finalize modes 1 and 2, all eight flag combinations of norm_apply on its three
kernels, the ReLU(BN) backward in train and eval mode on its five kernels with the centred form of its sums, the whole interface
of zt_partial_reduce_f32, the ticket pool, and the host-side argument checks.

Every output buffer is pre-filled with a sentinel.  References are fp64 on the same operands (bf16 cases: on the bf16-rounded
operands).  Each test prints the figure it measured ("NORM ..." lines, visible with -s) before it asserts.

Tolerances
  fp32 statistics: scale, rstd relative 5e-6; shift, mean 5e-6 * (1 + |ref|).  Statistics of bf16 inputs are held to the same
    figures: the sums are fp32 either way.
  partial rows, summed over the blocks in fp64, against the fp64 sum S and sum of squares: a row entry is an fp32 sum of at most
    chunk = ceil(HW / nblk) terms, accumulated as ceil(chunk / R) terms per thread and a fold of the R pixel rows of the workgroup
    (R = 256 / (C / 4), or 256 / (C / 8) on the bf16 16-byte kernel).  Every addition rounds by at most 2^-24 of a running sum that
    sum |x| bounds, so |got - S| <= depth * 2^-24 * sum |x| with depth = ceil(chunk / R) + R + 2 (the larger over both R; + 2: the
    product's rounding and second-order terms).  Reported as a fraction of that bound ("part"), which must not exceed 1.
  fp32 apply / backward outputs: 2e-5 absolute on unit-scale data (test_norms's figure).
  dgamma, dbeta, sums: 1e-5 * max |ref|.
  bf16 outputs: the project's bf16 contract as in test_norms_bf16_fast_path, max(|got - ref| - |ref| * 2^-8) < 1e-3.

ReLU mask.  The device evaluates z * scale + shift > 0 in fp32 -- as a multiply and an add in a build with contraction off (the
Makefiles' setting), as one fma where a compiler contracts it -- so an element whose BatchNorm output is within rounding of zero may
legitimately flip.  No element is excluded: the inputs are constructed (offending elements of z redrawn, reference recomputed)
until min |BN output| >= 1e-3 in the fp64 reference, and that is asserted before anything is compared.

Ill-conditioned statistics (test_ill_conditioned_statistics).  The kernels keep sum and sum of squares in fp32 per workgroup and
combine them in fp64, so the relative error of rstd grows with (mean / std)^2: about 0.4 * 2^-24 * (mean / std)^2 on the emulator.
The test pins that with the bound 4 * 2^-24 * (1 + (mean / std)^2) -- two to three fp32 roundings per accumulated term, chains of
HW / (nblk * R) terms plus R folds, errors adding as a random walk -- and checks that the normalised output x * scale + shift stays
within 2e-5 * (1 + mean / std) of fp64: there the errors of scale and shift cancel ((x - mean) * rstd only sees the relative
error of rstd), which is why nobody needs to "fix" the statistics with a centred second pass.  Measured relative error of rstd
(two-launch / one-launch) and error of the output, C = 64 fp32:
  mean/std   map        emu rstd              emu out    hip rstd              hip out     bounds (rstd, out)
  0          64x64      5.93e-08 / 5.93e-08   4.05e-07   5.93e-08 / 5.93e-08   4.05e-07    2.38e-07, 2.0e-05
  10         64x64      3.01e-06 / 3.01e-06   1.15e-05   3.01e-06 / 3.01e-06   1.15e-05    2.41e-05, 2.2e-04
  100        64x64      2.26e-04 / 2.26e-04   8.14e-04   2.26e-04 / 2.26e-04   8.14e-04    2.38e-03, 2.02e-03
  10         128x128    1.63e-06 / 1.63e-06   6.95e-06   1.63e-06 / 1.63e-06   6.95e-06    2.41e-05, 2.2e-04
The chip and the emulator agree to every printed digit: both builds keep contraction off and the kernels fix their summation order.

Largest figures measured over the module, gfx950 and emulator alike to every printed digit, each with its bound in brackets:
  statistics (sections 1, 2, 6): 6.77e-07 at C = 1024, 5 x 7 (5e-6); partial rows 0.183 of their bound at C = 96, 5 x 7 (1);
    the gpu-only 1024 x 1024 case: 4.12e-08 and 0.00078
  norm_apply: fp32 7.63e-07 (2e-5); bf16 excess 3.52e-08 (1e-3)
  backward: fp32 dz 3.57e-07 (2e-5); bf16 dz excess 6.09e-10 (1e-3); sums / dgamma / dbeta 2.43e-07 * max |ref| (1e-5 * max |ref|)
  partial reduce: bit-equal in every case; an fp32 combine in row order would differ in 3 to 4 of the 5 columns from nblk = 255 on
The emulator run of the module takes about 5 s after the emulator is built, the gfx950 run about 2 s."""
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

SENT = -768.0            # exact in bf16 and fp32; no kernel under test produces it
FILL = 1000.0            # what the channels outside a sliced input hold: exact in bf16, ruins any statistic it leaks into
STAT_TOL = 5e-6
F32_TOL = 2e-5
SUM_TOL = 1e-5
BF16_TOL = 1e-3
F32, BF16 = torch.float32, torch.bfloat16


def _CV():
    return import_module("zero-tig_amd.ops").CV


def _stream(dev):
    return import_module("zero-tig_amd.lib").current_stream(dev)


def _sent(shape, dtype, dev):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


def _report(what, case, **figs):
    print("NORM %s [%s] %s" % (what, case, " ".join("%s=%.3g" % kv for kv in figs.items())))


def _rel(got, ref):
    ref = ref.to(got.device)
    return float(((got.double() - ref).abs() / ref.abs()).max())


def _mix(got, ref):
    ref = ref.to(got.device)
    return float(((got.double() - ref).abs() / (1 + ref.abs())).max())


def _maxabs(got, ref):
    return float((got.double() - ref.to(got.device)).abs().max())


def _excess(got, ref):
    """the bf16 contract's left-hand side"""
    ref = ref.to(got.device)
    return float(((got.double() - ref).abs() - ref.abs() * 2.0 ** -8).max())


def _place(x, off, ld, dev, fill):
    """x [N,H,W,C] -> a [N,H,W,ld] buffer with x in channels [off, off + C) and `fill` elsewhere, and the channel view of x"""
    N, H, W, C = x.shape
    buf = torch.full((N, H, W, ld), fill, dtype=x.dtype)
    buf[..., off:off + C] = x
    buf = buf.to(dev)
    return buf, _CV()(buf, off, C)


def _outside_is(buf, off, C, value):
    return bool((buf[..., :off] == value).all()) and bool((buf[..., off + C:] == value).all())


def _dt(v):
    return 1 if v.t.dtype == BF16 else 0


def _chan_stats(ops, v, nblk):
    part = _sent((v.N, nblk, 2, v.C), F32, v.t.device)
    ops.lib.call("zt_chan_stats_nhwc", v.ptr, _dt(v), v.ld, v.N, v.H * v.W, v.C, nblk, part, _stream(v.t.device))
    return part


def _one_launch(ops, v, nblk, eps):
    dev = v.t.device
    part, scale, shift = _sent((v.N, nblk, 2, v.C), F32, dev), _sent((v.N, v.C), F32, dev), _sent((v.N, v.C), F32, dev)
    tick = torch.zeros(v.N, dtype=torch.int32, device=dev)
    ops.lib.call("zt_instance_norm_stats", v.ptr, _dt(v), v.ld, v.N, v.H * v.W, v.C, nblk, part, eps, tick, scale, shift, _stream(dev))
    assert int(tick.abs().sum()) == 0                          # the counters are handed back at zero
    return part, scale, shift


def _finalize(ops, dev, part, nblk, N, C, count, eps, mode, gamma=None, beta=None, rm=None, rv=None, nbt=None, momentum=0.1):
    """-> scale, shift, mean_out, rstd_out [N, C]"""
    outs = [_sent((N, C), F32, dev) for _ in range(4)]
    ops.lib.call("zt_norm_finalize_f32", part, nblk, N, C, count, eps, mode, gamma, beta, rm, rv, nbt, momentum, *outs, _stream(dev))
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# 1. statistics: chan_stats + norm_finalize mode 0, and instance_norm_stats in one launch, against fp64 mean and biased variance
# ---------------------------------------------------------------------------------------------------------------------
def _depth(C, chunk):
    rs = [256 // (C // 4)] + ([256 // (C // 8)] if C % 8 == 0 and 256 % (C // 8) == 0 else [])
    return max((chunk + R - 1) // R + R for R in rs) + 2


def _stats_case(ops, dev, name, kind, C, H, W, nblk=None, off=None, eps=1e-5):
    N, HW = 2, H * W
    g = torch.Generator().manual_seed(7919 * C + 31 * H + W + (off or 0))
    x = torch.randn(N, H, W, C, generator=g) * 1.5 + torch.tensor([0.4, -1.1]).view(N, 1, 1, 1) + 0.5 * torch.randn(1, 1, 1, C, generator=g)
    if kind == "bf16":
        x = x.bfloat16()
    buf, v = _place(x, off or 0, C + 16 if off is not None else C, dev, FILL)
    nb = ops._nblk(HW) if nblk is None else nblk
    x64 = v.t[..., v.off:v.off + C].double()                    # the reference runs where the data is
    mean, var = x64.mean((1, 2)), x64.var((1, 2), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    s1, s2, a1 = x64.sum((1, 2)), (x64 * x64).sum((1, 2)), x64.abs().sum((1, 2))
    chunk = (HW + nb - 1) // nb
    bound = _depth(C, chunk) * 2.0 ** -24
    empty = [b for b in range(nb) if b * chunk >= HW]
    case = "%s %s c%d %dx%d nblk%d%s" % (name, kind, C, H, W, nb, "" if off is None else " off%d" % off)

    part = _chan_stats(ops, v, nb)
    sc, sh, mu, rs = _finalize(ops, dev, part, nb, N, C, HW, eps, 0)
    part1, sc1, sh1 = _one_launch(ops, v, nb, eps)
    figs = {}
    for tag, p in (("two", part), ("one", part1)):
        ps = p.double().sum(1)
        figs["part_" + tag] = float(torch.maximum((ps[:, 0] - s1).abs() / (bound * a1), (ps[:, 1] - s2).abs() / (bound * s2)).max())
    figs.update(scale=_rel(sc, rstd), shift=_mix(sh, -mean * rstd), mean=_mix(mu, mean), rstd=_rel(rs, rstd),
                scale1=_rel(sc1, rstd), shift1=_mix(sh1, -mean * rstd))
    _report("stats", case, empty_rows=len(empty), **figs)
    assert figs["part_two"] <= 1.0 and figs["part_one"] <= 1.0, figs
    assert torch.equal(part, part1)                            # the same kernel; the tail only reads the rows
    if empty:
        assert bool((part[:, empty] == 0).all()) and bool((part1[:, empty] == 0).all())
    for k in ("scale", "shift", "mean", "rstd", "scale1", "shift1"):
        assert figs[k] <= STAT_TOL, (k, figs[k])
    assert _outside_is(buf, off or 0, C, FILL)


# 5 x 7: auto nblk = 1;  9 x 14 in 4 blocks: chunk 32, the last one 30 pixels;  5 x 7 in 64 blocks: chunk 1, 29 empty ranges, and
# more than 8 * G rows in the tail (G = 256 / C below 256 channels, 1 above) from C = 12 on and in the finalize kernel (G = 1024 / C,
# 4 from 256 channels on) from C = 256 on.  C = 4, 8: Q = 1, 2 -> R = 256 pixel rows;  12: Q = 3, R = 85, one idle thread;
# 384, 1024: a second and a fourth pass over 256 channels (cbase > 0), 384 leaving half a pass unused.
STATS_F32 = [(C, H, W, nb) for C in (4, 8, 12, 96, 256, 384, 1024) for H, W, nb in ((5, 7, None), (9, 14, 4), (5, 7, 64))]
STATS_F32.append((64, 128, 128, None))                         # auto nblk = 256 > 8 * G = 128 in the finalize kernel


@pytest.mark.parametrize("case", STATS_F32, ids=lambda c: "c%d_%dx%d_nblk%s" % c)
def test_stats_f32(backend, case):
    ops, dev, name = backend
    C, H, W, nb = case
    _stats_case(ops, dev, name, "f32", C, H, W, nb)


# generic bf16 kernel: HW < 4096, or 256 % (C / 8) != 0 (C = 48: 6 octets).  16-byte kernel at 65 x 67 = 4355 pixels in 68 blocks of
# 65: ragged against NPIX * R (R = 256, 32, 16 for C = 8, 64, 128), against the chunk, and block 67 starts at pixel 4355: empty.
STATS_BF16 = [(96, 23, 40), (48, 65, 67), (8, 65, 67), (64, 65, 67), (128, 65, 67)]


@pytest.mark.parametrize("case", STATS_BF16, ids=lambda c: "c%d_%dx%d" % c)
def test_stats_bf16(backend, case):
    ops, dev, name = backend
    _stats_case(ops, dev, name, "bf16", *case)


# channel slices of a buffer 16 channels wider, the rest of it holding 1000.0.  Offset 8: 16-byte aligned rows in both types.
# bf16 at offset 4: rows 8 bytes off, so the 65 x 67 case must fall to the generic kernel.
STATS_SLICED = [("f32", 12, 5, 7, None, 8), ("f32", 96, 9, 14, 4, 8), ("bf16", 96, 23, 40, None, 8), ("bf16", 96, 23, 40, None, 4),
                ("bf16", 64, 65, 67, None, 8), ("bf16", 64, 65, 67, None, 4)]


@pytest.mark.parametrize("case", STATS_SLICED, ids=lambda c: "%s_c%d_%dx%d_nblk%s_off%d" % c)
def test_stats_sliced(backend, case):
    ops, dev, name = backend
    _stats_case(ops, dev, name, *case)


@pytest.mark.gpu
def test_stats_bf16_megapixel(hip_ops):
    """HW = 2^20: the wrapper's partial-row count for maps of a megapixel and more (1024 unless tuned otherwise)"""
    ops, dev = hip_ops
    assert ops._nblk(1 << 20) == import_module("zero-tig_amd.ops")._NBLK_BIG
    _stats_case(ops, dev, "hip", "bf16", 8, 1024, 1024)


# ---------------------------------------------------------------------------------------------------------------------
# 2. finalize modes 1 (train BatchNorm, running statistics) and 2 (eval BatchNorm, partial = NULL) against fp64 F.batch_norm
# ---------------------------------------------------------------------------------------------------------------------
def _bn_params(C, g):
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    return gam, bet, rm, rv


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("momentum", [0.1, 0.25])
@pytest.mark.parametrize("C", [64, 384])
def test_finalize_train(backend, C, momentum, eps):
    """three consecutive train-mode calls: scale / shift / mean / rstd of the batch, running mean, running variance with the
    unbiased factor HW / (HW - 1), and the counter growing by exactly one per call"""
    ops, dev, name = backend
    H, W = 9, 14
    HW = H * W
    g = torch.Generator().manual_seed(100 + C)
    gam, bet, rm, rv = _bn_params(C, g)
    rm64, rv64 = rm.double(), rv.double()
    gd, bd, rmd, rvd = (t.to(dev) for t in (gam, bet, rm, rv))
    nbt = torch.full((), 5, dtype=torch.int64, device=dev)
    worst = dict(scale=0.0, shift=0.0, mean=0.0, rstd=0.0, rmean=0.0, rvar=0.0)
    for call in range(3):
        x = torch.randn(1, H, W, C, generator=g) * (1.0 + 0.5 * call) + 0.3 * call + 0.5 * torch.randn(1, 1, 1, C, generator=g)
        x64 = x.double()
        F.batch_norm(x64.permute(0, 3, 1, 2), rm64, rv64, gam.double(), bet.double(), True, momentum, eps)   # updates rm64 / rv64
        mean, var = x64.mean((1, 2)), x64.var((1, 2), unbiased=False)
        rstd = 1.0 / torch.sqrt(var + eps)
        scale = gam.double() * rstd
        part = _chan_stats(ops, _CV()(x.to(dev)), 4)
        sc, sh, mu, rs = _finalize(ops, dev, part, 4, 1, C, HW, eps, 1, gd, bd, rmd, rvd, nbt, momentum)
        figs = dict(scale=_rel(sc, scale), shift=_mix(sh, bet.double() - mean * scale), mean=_mix(mu, mean), rstd=_rel(rs, rstd),
                    rmean=_mix(rmd, rm64), rvar=_mix(rvd, rv64))
        worst = {k: max(worst[k], figs[k]) for k in worst}
        assert int(nbt) == 6 + call, int(nbt)
    _report("finalize-train", "%s c%d momentum %g eps %g" % (name, C, momentum, eps), **worst)
    for k, f in worst.items():
        assert f <= STAT_TOL, (k, f)


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("C", [64, 384])
def test_finalize_eval(backend, C, eps):
    """mode 2 reads no partials (NULL, nblk 0) and leaves the running statistics and the counter bit for bit as they were"""
    ops, dev, name = backend
    g = torch.Generator().manual_seed(200 + C)
    gam, bet, rm, rv = _bn_params(C, g)
    gd, bd, rmd, rvd = (t.to(dev) for t in (gam, bet, rm, rv))
    nbt = torch.full((), 5, dtype=torch.int64, device=dev)
    sc, sh, mu, rs = _finalize(ops, dev, None, 0, 1, C, 1, eps, 2, gd, bd, rmd, rvd, nbt, 0.1)
    x64 = torch.randn(1, C, 3, 5, generator=g).double()
    y = F.batch_norm(x64, rm.double(), rv.double(), gam.double(), bet.double(), False, 0.1, eps)
    rstd = 1.0 / torch.sqrt(rv.double() + eps)
    scale = gam.double() * rstd
    shift = bet.double() - rm.double() * scale
    assert float((x64 * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1) - y).abs().max()) < 1e-12    # scale / shift are F.batch_norm's
    figs = dict(scale=_rel(sc[0], scale), shift=_mix(sh[0], shift), mean=_mix(mu[0], rm.double()), rstd=_rel(rs[0], rstd))
    _report("finalize-eval", "%s c%d eps %g" % (name, C, eps), **figs)
    for k, f in figs.items():
        assert f <= STAT_TOL, (k, f)
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv) and int(nbt) == 5


# ---------------------------------------------------------------------------------------------------------------------
# 3. norm_apply: y = [outer_relu]([res +] [inner_relu](x * scale + shift)), all eight flag combinations, N = 2 with a scale / shift
# row per sample, input / residual / output as slices of three different widths
# ---------------------------------------------------------------------------------------------------------------------
# (kind, C, H, W, ((off, ld - C) of x, res, y)).  "bf16x8" = the 16-byte kernel: HW >= 4096, every offset and width a multiple
# of 8; 65 * 67 % 4 = 3, so the last pixel group is ragged, and 48 and 96 channels are 6 and 12 octets per pixel.
APPLY = [("f32", 12, 9, 14, ((4, 16), (8, 8), (4, 12))), ("f32", 96, 9, 14, ((4, 16), (8, 8), (4, 12))),
         ("bf16", 48, 23, 40, ((4, 16), (8, 8), (4, 12)))]
APPLY += [("bf16x8", C, 65, 67, ((8, 16), (0, 8), (16, 24))) for C in (8, 48, 64, 96)]


@pytest.mark.parametrize("case", APPLY, ids=lambda c: "%s_c%d_%dx%d" % c[:4])
def test_norm_apply(backend, case):
    ops, dev, name = backend
    kind, C, H, W, places = case
    N = 2
    dtype = F32 if kind == "f32" else BF16
    g = torch.Generator().manual_seed(300 + C + H)
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + 0.2).to(dtype)
    res = torch.randn(N, H, W, C, generator=g).to(dtype)
    sign = torch.where(torch.rand(N, C, generator=g) < 0.3, -1.0, 1.0)
    scale, shift = ((torch.rand(N, C, generator=g) + 0.5) * sign).contiguous(), torch.randn(N, C, generator=g)
    (xo, xw), (ro, rw), (yo, yw) = places
    xbuf, xv = _place(x, xo, C + xw, dev, FILL)
    rbuf, rv = _place(res, ro, C + rw, dev, FILL)
    scd, shd = scale.to(dev), shift.to(dev)
    sc64, sh64 = scale.double().view(N, 1, 1, C), shift.double().view(N, 1, 1, C)
    worst = -1e30
    for combo in range(8):
        inner, outer, with_res = bool(combo & 1), bool(combo & 2), bool(combo & 4)
        ybuf = _sent((N, H, W, C + yw), dtype, dev)
        ops.norm_apply(xv, scd, shd, out=_CV()(ybuf, yo, C), res=rv if with_res else None, inner_relu=inner, outer_relu=outer)
        ref = x.double() * sc64 + sh64
        if inner:
            ref = ref.clamp_min(0)
        if with_res:
            ref = ref + res.double()
        if outer:
            ref = ref.clamp_min(0)
        got = ybuf[..., yo:yo + C]
        fig, tol = (_maxabs(got, ref), F32_TOL) if kind == "f32" else (_excess(got, ref), BF16_TOL)
        worst = max(worst, fig)
        _report("apply", "%s %s c%d %dx%d inner%d outer%d res%d" % (name, kind, C, H, W, inner, outer, with_res), err=fig, tol=tol)
        assert fig < tol, (combo, fig)
        assert _outside_is(ybuf, yo, C, SENT)
    assert _outside_is(xbuf, xo, C, FILL) and _outside_is(rbuf, ro, C, FILL)


# ---------------------------------------------------------------------------------------------------------------------
# 4. backward of ReLU(BN(z)), train mode and eval_mode, against fp64 autograd; the centred form of the sums
# ---------------------------------------------------------------------------------------------------------------------
MASK_MARGIN = 1e-3


def _bwd_reference(z, dy, gam, bet, rm, rv, eval_mode, eps):
    z64 = z.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    bn = F.batch_norm(z64.permute(0, 3, 1, 2), rm.double(), rv.double(), g64, b64, not eval_mode, 0.0, eps).permute(0, 2, 3, 1)
    (F.relu(bn) * dy.double()).sum().backward()
    return bn.detach(), z64.grad, g64.grad, b64.grad


def _bwd_inputs(kind, C, H, W, eval_mode, eps):
    """operands whose fp64 BatchNorm output stays MASK_MARGIN away from zero in every element (see the module docstring)"""
    rnd = (lambda t: t) if kind == "f32" else (lambda t: t.bfloat16())
    g = torch.Generator().manual_seed(400 + 3 * C + H + int(eval_mode))
    z, dy = rnd(torch.randn(1, H, W, C, generator=g) * 1.7 + 0.3), rnd(torch.randn(1, H, W, C, generator=g))
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    rm, rv = torch.randn(C, generator=g) * 0.2 + 0.3, torch.rand(C, generator=g) + 2.0
    for redraws in range(20):
        bn, dz, dgam, dbet = _bwd_reference(z, dy, gam, bet, rm, rv, eval_mode, eps)
        bad = bn.abs() < MASK_MARGIN
        if not bool(bad.any()):
            break
        z[bad] = rnd(torch.randn(int(bad.sum()), generator=g) * 1.7 + 0.3)
    assert float(bn.abs().min()) >= MASK_MARGIN, "no element may sit within rounding of the ReLU's kink"
    return z, dy, gam, bet, rm, rv, bn, dz, dgam, dbet, redraws


# fp32 and generic bf16 (HW < 4096): offsets that are multiples of 4 only.  bf16 at 65 x 67 on multiples of 8: 64 channels take the
# 16-byte reduce and apply kernels; 48 channels (6 octets, 256 % 6 != 0) are refused by both and fall back to the generic ones.
BWD = [("f32", 12, 10, 13), ("f32", 64, 19, 37), ("bf16", 64, 19, 37), ("bf16", 64, 65, 67), ("bf16", 48, 65, 67)]


@pytest.mark.parametrize("eval_mode", [False, True], ids=["train", "eval"])
@pytest.mark.parametrize("case", BWD, ids=lambda c: "%s_c%d_%dx%d" % c)
def test_bn_relu_bwd(backend, case, eval_mode):
    ops, dev, name = backend
    kind, C, H, W = case
    HW, eps = H * W, 1e-5
    z, dy, gam, bet, rm, rv, bn, dz_ref, dgam_ref, dbet_ref, redraws = _bwd_inputs(kind, C, H, W, eval_mode, eps)
    wide = HW >= 4096
    (go, gw), (zo, zw), (oo, ow) = ((8, 16), (8, 8), (16, 24)) if wide else ((4, 16), (8, 8), (4, 12))
    dybuf, dyv = _place(dy, go, C + gw, dev, FILL)
    zbuf, zv = _place(z, zo, C + zw, dev, FILL)
    gd, bd, rmd, rvd = (t.to(dev) for t in (gam, bet, rm, rv))
    # the forward's statistics, as the engine takes them
    if eval_mode:
        sc, sh, mu, rs = _finalize(ops, dev, None, 0, 1, C, 1, eps, 2, gd, bd, rmd, rvd)
    else:
        nb = ops._nblk(HW)
        sc, sh, mu, rs = _finalize(ops, dev, _chan_stats(ops, zv, nb), nb, 1, C, HW, eps, 1, gd, bd, rmd, rvd, None, 0.1)
    # two launches + apply, as Ops.bn_relu_bwd issues them, with every output visible
    nb = ops._nblk(HW)
    part, sums = _sent((nb, 2, C), F32, dev), _sent((2, C), F32, dev)
    dgam, dbet = torch.full((C,), 3.0, device=dev), torch.full((C,), 3.0, device=dev)
    dzbuf = _sent((1, H, W, C + ow), z.dtype, dev)
    s = _stream(dev)
    ops.lib.call("zt_bn_bwd_reduce", dyv.ptr, _dt(zv), dyv.ld, zv.ptr, zv.ld, sc, sh, mu, rs, HW, C, nb, part, s)
    ops.lib.call("zt_bn_bwd_sums_f32", part, nb, C, dbet, dgam, sums, s)
    ops.lib.call("zt_bn_bwd_apply", dyv.ptr, _dt(zv), dyv.ld, zv.ptr, zv.ld, sc, sh, mu, rs, sums, dzbuf.data_ptr() + oo * z.element_size(),
                 C + ow, HW, C, int(eval_mode), s)
    # the centred form: [512][2][C] partials as the data-gradient kernel leaves them, (sum g, sum g (z - mean)) over 5 rows
    mean64 = rm.double() if eval_mode else z.double().mean((0, 1, 2))
    gm = torch.where(bn > 0, dy.double(), torch.zeros((), dtype=torch.float64))
    tot = torch.stack([gm.sum((0, 1, 2)), (gm * (z.double() - mean64)).sum((0, 1, 2))])         # [2, C]
    cpart = torch.zeros(512, 2, C)
    cpart[:5] = (torch.tensor([0.3, -0.2, 0.5, 0.25, 0.15], dtype=torch.float64).view(5, 1, 1) * tot).float()
    dgam_c, dbet_c = torch.full((C,), 3.0, device=dev), torch.full((C,), 3.0, device=dev)
    dzbuf_c = _sent((1, H, W, C + ow), z.dtype, dev)
    ops.bn_relu_bwd(dyv, zv, sc, sh, mu, rs, dgam_c, dbet_c, out=_CV()(dzbuf_c, oo, C), eval_mode=eval_mode, part=cpart.to(dev))

    sums_ref = torch.stack([dbet_ref, dgam_ref])
    stol = SUM_TOL * float(sums_ref.abs().max())
    figs = dict(sums=_maxabs(sums, sums_ref), dgamma=_maxabs(dgam.double() - 3.0, dgam_ref), dbeta=_maxabs(dbet.double() - 3.0, dbet_ref),
                dgamma_c=_maxabs(dgam_c.double() - 3.0, dgam_ref), dbeta_c=_maxabs(dbet_c.double() - 3.0, dbet_ref))
    dz_err = _maxabs if kind == "f32" else _excess
    dz_tol = F32_TOL if kind == "f32" else BF16_TOL
    figs.update(dz=dz_err(dzbuf[..., oo:oo + C], dz_ref), dz_c=dz_err(dzbuf_c[..., oo:oo + C], dz_ref))
    _report("bn-bwd", "%s %s c%d %dx%d %s" % (name, kind, C, H, W, "eval" if eval_mode else "train"), redraws=redraws,
            min_bn=float(bn.abs().min()), sum_tol=stol, dz_tol=dz_tol, **figs)
    for k in ("sums", "dgamma", "dbeta", "dgamma_c", "dbeta_c"):
        assert figs[k] <= stol, (k, figs[k], stol)
    assert figs["dz"] < dz_tol and figs["dz_c"] < dz_tol, figs
    assert _outside_is(dzbuf, oo, C, SENT) and _outside_is(dzbuf_c, oo, C, SENT)
    assert _outside_is(dybuf, go, C, FILL) and _outside_is(zbuf, zo, C, FILL)


# ---------------------------------------------------------------------------------------------------------------------
# 5. zt_partial_reduce_f32: out[j] (+)= sum_b partial[b * stride + j], combined in fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 255, 256, 257, 1000])
def test_partial_reduce(backend, nblk):
    """integer-valued partials of mixed sign between 1 and 2^30: any fp64 summation order is exact (|sum| < 2^40), an fp32 one
    is not, so the result must equal float32(exact sum) bit for bit.  stride 8 > n = 5, the unused columns holding NaN."""
    ops, dev, name = backend
    n, stride = 5, 8
    g = torch.Generator().manual_seed(500 + nblk)
    mant = torch.randint(1, 1024, (nblk, n), generator=g).double()
    val = mant * 2.0 ** torch.randint(0, 21, (nblk, n), generator=g).double() * torch.where(torch.rand(nblk, n, generator=g) < 0.5, -1.0, 1.0)
    assert float(val.abs().max()) < 2.0 ** 30
    part = torch.full((nblk, stride), float("nan"))
    part[:, :n] = val.float()
    assert torch.equal(part[:, :n].double(), val)
    exact = val.sum(0).float()                                  # fp64 -> fp32 rounds to nearest even, as the kernel's cast does
    fp32_order = torch.zeros(n)
    for b in range(nblk):
        fp32_order = fp32_order + part[b, :n]                   # what an fp32 combine would give: reported, to show the data bites
    pd, ed = part.to(dev), exact.to(dev)
    start = torch.tensor([7.0, -3.0e9, 0.5, 1.0e12, -1.0])

    def run(out, accumulate, out2):
        ops.partial_reduce(pd, nblk, stride, n, out=out, accumulate=accumulate, out2=out2)

    o = torch.cat([start, torch.full((3,), SENT)]).to(dev)
    run(o, False, None)
    ok_plain = torch.equal(o[:n], ed) and bool((o[n:] == SENT).all())
    o = torch.cat([start, torch.full((3,), SENT)]).to(dev)
    run(o, True, None)
    ok_acc = torch.equal(o[:n].cpu(), start + exact) and bool((o[n:] == SENT).all())
    o2 = _sent((n + 3,), F32, dev)
    run(None, False, o2)
    ok_out2 = torch.equal(o2[:n], ed) and bool((o2[n:] == SENT).all())
    o, o2 = torch.cat([start, torch.full((3,), SENT)]).to(dev), _sent((n + 3,), F32, dev)
    run(o, True, o2)
    ok_both = torch.equal(o[:n].cpu(), start + exact) and torch.equal(o2[:n], ed) and bool((o[n:] == SENT).all()) and bool((o2[n:] == SENT).all())
    _report("partial-reduce", "%s nblk%d" % (name, nblk), plain=ok_plain, accumulate=ok_acc, out2=ok_out2, both=ok_both,
            fp32_combine_would_differ=float((fp32_order != exact).sum()))
    assert ok_plain and ok_acc and ok_out2 and ok_both


# ---------------------------------------------------------------------------------------------------------------------
# 6. the ticket pool of Ops.instance_norm_stats
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("f32", 64, 23, 40), ("bf16", 64, 65, 67)], ids=lambda c: "%s_c%d_%dx%d" % c)
def test_ticket_pool(backend, case):
    """counters back at zero after every call; the cursor wraps at 4096 (N = 2 from 4095 does not fit) and the result is still
    right; three back-to-back calls on one tensor are bit-identical"""
    ops, dev, name = backend
    kind, C, H, W = case
    g = torch.Generator().manual_seed(600 + C + H)
    x = torch.randn(2, H, W, C, generator=g) * 1.5 + torch.tensor([0.4, -1.1]).view(2, 1, 1, 1)
    if kind == "bf16":
        x = x.bfloat16()
    xd = x.to(dev)
    x64 = x.double()
    mean, rstd = x64.mean((1, 2)), 1.0 / torch.sqrt(x64.var((1, 2), unbiased=False) + 1e-5)
    sc0, sh0 = ops.instance_norm_stats(xd)
    pool = ops._tickets[xd.device]
    assert int(pool[0].abs().sum()) == 0
    pool[1] = 4095
    sc, sh = ops.instance_norm_stats(xd)
    wrapped_to = pool[1]
    zero_after_wrap = int(pool[0].abs().sum()) == 0
    figs = dict(scale=_rel(sc, rstd), shift=_mix(sh, -mean * rstd))
    same = torch.equal(sc, sc0) and torch.equal(sh, sh0)
    for _ in range(3):
        sc1, sh1 = ops.instance_norm_stats(xd)
        same = same and torch.equal(sc1, sc0) and torch.equal(sh1, sh0) and int(pool[0].abs().sum()) == 0
    _report("tickets", "%s %s c%d %dx%d" % (name, kind, C, H, W), cursor_after_wrap=wrapped_to, bit_identical=same, **figs)
    assert wrapped_to == 2 and zero_after_wrap and pool[1] == 8
    assert figs["scale"] <= STAT_TOL and figs["shift"] <= STAT_TOL, figs
    assert same


# ---------------------------------------------------------------------------------------------------------------------
# 7. ill-conditioned statistics: pinned, not fixed (see the module docstring)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(0, 64, 64), (10, 64, 64), (100, 64, 64), (10, 128, 128)], ids=lambda c: "ratio%d_%dx%d" % c)
def test_ill_conditioned_statistics(backend, case):
    ops, dev, name = backend
    ratio, H, W = case
    C, HW, eps = 64, H * W, 1e-5
    g = torch.Generator().manual_seed(700 + ratio + H)
    x = torch.randn(1, H, W, C, generator=g) + float(ratio)
    xd = x.to(dev)
    v = _CV()(xd)
    x64 = x.double()
    mean, rstd = x64.mean((1, 2)), 1.0 / torch.sqrt(x64.var((1, 2), unbiased=False) + eps)
    nb = ops._nblk(HW)
    sc, sh, mu, rs = _finalize(ops, dev, _chan_stats(ops, v, nb), nb, 1, C, HW, eps, 0)
    _, sc1, sh1 = _one_launch(ops, v, nb, eps)
    y = ops.norm_apply(v, sc, sh, out=_sent((1, H, W, C), F32, dev))
    bound, ybound = 4 * 2.0 ** -24 * (1 + ratio * ratio), 2e-5 * (1 + ratio)
    figs = dict(rstd=_rel(rs, rstd), rstd1=_rel(sc1, rstd), out=_maxabs(y, (x64 - mean.view(1, 1, 1, C)) * rstd.view(1, 1, 1, C)))
    _report("ill-conditioned", "%s mean/std %d %dx%d nblk%d" % (name, ratio, H, W, nb), bound=bound, out_bound=ybound, **figs)
    assert figs["rstd"] <= bound and figs["rstd1"] <= bound, figs
    assert figs["out"] <= ybound, figs


# ---------------------------------------------------------------------------------------------------------------------
# 8. host-side argument checks: every call below is rejected by a ZT_REQUIRE before anything is launched
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    ops, dev, name = backend
    C, HW = 8, 6
    f = lambda *shape: _sent(shape, F32, dev)
    dy, z, dz, part, sums = f(1, 2, 3, C), f(1, 2, 3, C), f(1, 2, 3, C), f(4, 2, C), f(2, C)
    sc, sh, mu, rs, gam, bet, rm, rv = (f(1, C) for _ in range(8))
    s = _stream(dev)
    rejected = {
        "bwd_reduce nblk 0": ("zt_bn_bwd_reduce", dy, 0, C, z, C, sc, sh, mu, rs, HW, C, 0, part, s),
        "bwd_reduce lddy % 4": ("zt_bn_bwd_reduce", dy, 0, C + 2, z, C, sc, sh, mu, rs, HW, C, 4, part, s),
        "bwd_reduce ldz % 4": ("zt_bn_bwd_reduce", dy, 0, C, z, C + 2, sc, sh, mu, rs, HW, C, 4, part, s),
        "bwd_apply lddy % 4": ("zt_bn_bwd_apply", dy, 0, C + 2, z, C, sc, sh, mu, rs, sums, dz, C, HW, C, 0, s),
        "bwd_apply ldz % 4": ("zt_bn_bwd_apply", dy, 0, C, z, C + 2, sc, sh, mu, rs, sums, dz, C, HW, C, 0, s),
        "bwd_apply lddz % 4": ("zt_bn_bwd_apply", dy, 0, C, z, C, sc, sh, mu, rs, sums, dz, C + 2, HW, C, 0, s),
        "bwd_apply HW 0": ("zt_bn_bwd_apply", dy, 0, C, z, C, sc, sh, mu, rs, sums, dz, C, 0, C, 0, s),
        "finalize count 0": ("zt_norm_finalize_f32", part, 4, 1, C, 0, 1e-5, 0, None, None, None, None, None, 0.1, sc, sh, mu, rs, s),
        "finalize nblk 0 mode 0": ("zt_norm_finalize_f32", part, 0, 1, C, HW, 1e-5, 0, None, None, None, None, None, 0.1, sc, sh, mu, rs, s),
        "finalize nblk 0 mode 1": ("zt_norm_finalize_f32", part, 0, 1, C, HW, 1e-5, 1, gam, bet, rm, rv, None, 0.1, sc, sh, mu, rs, s),
        "finalize count 1 mode 1": ("zt_norm_finalize_f32", part, 4, 1, C, 1, 1e-5, 1, gam, bet, rm, rv, None, 0.1, sc, sh, mu, rs, s),
    }
    for what, call in rejected.items():
        with pytest.raises(RuntimeError, match="code 1001"):
            ops.lib.call(*call)
        _report("rejected", "%s %s" % (name, what), code=1001)
    for t in (dy, z, dz, part, sums, sc, sh, mu, rs, gam, bet, rm, rv):
        assert bool((t == SENT).all())                          # nothing ran
