"""The two ends of RaftPlan.update_cache, one launch at a time: the kernels that turn the cached frame and the current frame into
RAFT's inputs (resize_bilinear, equalize_prepare, raft_pack_input / zt_raft_pack_pair, the 7x7 stem), the fused correlation
volume + pyramid they feed, and the backward warp of the cache (both warp kernels).  The refinement loop in between is
tests/test_raft_loop.py's.

References.  The bilinear kernels promise one fixed sequence of fp32 operations (zt_lin_index, row = fma(a, w0, b * w1),
out = fma(r0, wy0, r1 * wy1); for the warp g = m / den - 1, ix = fma(g + 1, size / 2, -0.5), four taps accumulated by fma).
oracle.bilinear_fma32 / warp_fma32 restate that sequence in plain torch and are exact at EVERY shape; resize and warp are compared
with them bit for bit.  ATen's CPU kernels give the same bits only at wide outputs, so the restatement is first pinned to
F.interpolate / oracle.warp_tensor / oracle.warp_taps where they agree (test_restatement_pinned_to_torch) and torch's values are
and taps are asserted against the kernels only for images at least 128 wide.  Integer kernels (equalisation, packing) are compared with torch
bit for bit; the bf16 stem under the bf16 contract of test_raft_loop (max(|got - ref| - |ref| 2^-8) < 2e-3, fp64 reference on the
bf16-rounded operands); the correlation volume within 2e-5 max|ref| of an fp64 product, and exactly on one-hot inputs.

Every output buffer is a larger allocation pre-filled with a sentinel, so a store outside the documented extent shows.  Each test
prints what it measured ("RAFTENDS <what> [<backend>] key=value", visible with -s) before it asserts.

Measured figures (torch 2.10 CPU, 8 threads, for the torch columns; "emu" = tests/hipemu on that CPU, "hip" = MI355X):
  * resize against the fp64 definition, in ulp of max|ref|, largest over RESIZE_SHAPES, 540 x 960 -> 181 x 320 and mul in {255, 1}:
    F.interpolate * mul 1.754 (CPU, at 5 x 130 -> 2 x 129, mul 255); kernel 1.754 on emu and on hip (same shape; 1.458 at 540p on
    hip).  The kernel is allowed twice torch's figure, RESIZE_DEF_ULP = 3.51.
  * smallest output width from which F.interpolate equals the restatement at every width tried up to 140, for 8 x 48 -> 21 x w:
    108 (CPU); none of the widths 40 .. 107 agrees.  Narrow shapes at which torch differed: (31,47)->(10,15), (8,8)->(3,5),
    (10,10)->(20,20), by one ulp.  The kernels are therefore compared with torch only from width 128 up.
  * warp, share of pixels with all four taps inside the image (the reference's own figure, the same on every backend), over the
    cases held to the covering condition: 0.55 - 0.96 at flow amplitude 2, 0.073 - 0.61 at amplitude 40 where 0.39 - 0.93 have a tap
    outside; the three cases of WARP_LOW_COVER: 0.106, 0.433, 0.019.
  * fused pyramid against the stand-alone pooling of its own level 0, largest difference as a share of the derived bound
    4 L u avgpool^L(|corr0|): 0.61 - 0.76 at the three small maps on emu, 0.61 - 0.71 on hip, 0.79 at 46 x 62 (hip); 0 on the one-hot inputs."""
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

SENT = -768.0            # exact in bf16 and fp32; no kernel under test produces it
ISENT = -7654321         # the same for int32 buffers
TAIL = 96                # elements of sentinel kept after (and, where alignment allows, before) every output
BF16_TOL = 2e-3          # test_conv_bf16's contract: max(|got - ref| - |ref| * 2^-8) < 2e-3
# fp32 F.interpolate(..) * mul sits 1.755 ulp(max|ref|) from the fp64 definition at worst over RESIZE_SHAPES and the 540p case (four
# roundings: two rows, the column, the product; each test prints its own figure); the kernel does the same roundings in another order
# and gets twice that
RESIZE_TORCH_ULP = 1.755
RESIZE_DEF_ULP = 2 * RESIZE_TORCH_ULP


def _stream(dev):
    return import_module("zero-tig_amd.lib").current_stream(dev)


def _report(what, name, **figs):
    print("RAFTENDS %s [%s] %s" % (what, name, " ".join("%s=%.4g" % kv for kv in figs.items())))


def _guarded(n, dtype, dev, head=0):
    """flat buffer of head + n + TAIL elements filled with the sentinel -> (whole buffer, the n elements a launch may write)"""
    buf = torch.full((head + n + TAIL,), ISENT if dtype == torch.int32 else SENT, dtype=dtype, device=dev)
    return buf, buf[head:head + n]


def _untouched(buf, n, head=0):
    s = ISENT if buf.dtype == torch.int32 else SENT
    return bool((buf[:head] == s).all()) and bool((buf[head + n:] == s).all())


def _ulp_of_max(ref):
    """one unit in the last place of fp32 at max|ref|"""
    m = float(ref.abs().max())
    return 2.0 ** (torch.frexp(torch.tensor(m, dtype=torch.float64))[1].item() - 1 - 23)


def _excess(got, ref):
    return float(((got.double() - ref).abs() - ref.abs() * 2.0 ** -8).max())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement is ATen's arithmetic where ATen is known to agree
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_pinned_to_torch(oracle):
    g = torch.Generator().manual_seed(11)
    for (H, W), (h, w) in (((8, 48), (21, 130)), ((31, 47), (10, 130)), ((544, 960), (181, 320)), ((45, 80), (136, 240))):
        x = torch.rand(1, 3, H, W, generator=g)
        assert torch.equal(oracle.bilinear_fma32(x, h, w), F.interpolate(x, (h, w), mode="bilinear")), (H, W, h, w)
    # where the agreement starts: F.interpolate on 8 x 48 -> 21 x w
    x = torch.rand(1, 3, 8, 48, generator=g)
    agree = {w: torch.equal(oracle.bilinear_fma32(x, 21, w), F.interpolate(x, (21, w), mode="bilinear")) for w in range(40, 141)}
    first = min(w for w in agree if all(agree[v] for v in range(w, 141)))
    _report("torch-agrees-from-width", "cpu", width=first, narrower_agreeing=sum(agree[w] for w in range(40, first)))
    assert first <= 128
    # the warp: values and tap indices, a 3 : 1 flow with padding (24 x 136 under 8 x 46), a ragged one and full resolution
    for (H, W, Hf, Wf) in ((24, 136, 8, 46), (21, 130, 8, 48), (136, 168, 136, 168)):
        flow = 3.0 * torch.randn(1, 2, Hf, Wf, generator=g)
        img = torch.rand(1, 3, H, W, generator=g)
        out, taps, _ = oracle.warp_fma32(flow, img)
        assert torch.equal(out, oracle.warp_tensor(flow, img)), (H, W, Hf, Wf)
        assert torch.equal(taps.to(torch.int32), oracle.warp_taps(flow, H, W)[0])


# ---------------------------------------------------------------------------------------------------------------------
# 2. resize_bilinear
# ---------------------------------------------------------------------------------------------------------------------
# (10,10)->(20,20) up-scales, (24,40)->(12,40) and (9,200)->(9,67) keep one axis (the fma sequence still runs, with weights 1 and 0),
# (30,50)->(30,50) copies, (5,130)->(2,129) has three column blocks of 64 with a ragged last one, (8,8)->(3,5) is one partial block
RESIZE_SHAPES = [((30, 50), (10, 16)), ((31, 47), (10, 15)), ((8, 8), (3, 5)), ((10, 10), (20, 20)), ((24, 40), (12, 40)), ((9, 200), (9, 67)),
                 ((30, 50), (30, 50)), ((5, 130), (2, 129))]
_rs = lambda s: "%dx%d-%dx%d" % (s[0] + s[1])


def _resize(ops, dev, x, h, w, mul):
    _, C, H, W = x.shape
    buf, out = _guarded(C * h * w, torch.float32, dev)
    ops.lib.call("zt_resize_bilinear_f32", x.to(dev), out, C, H, W, h, w, float(mul), _stream(dev))
    assert _untouched(buf, C * h * w)                          # the output is exactly C * h * w floats
    via_ops = ops.resize_bilinear(x.to(dev), h, w, mul)
    assert tuple(via_ops.shape) == (1, C, h, w) and torch.equal(via_ops.view(-1), out)
    return out.view(1, C, h, w).cpu()


def _resize_checks(ops, dev, name, oracle, shape, mul):
    (H, W), (h, w) = shape
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W + h))
    got = _resize(ops, dev, x, h, w, mul)
    want = oracle.bilinear_fma32(x, h, w, mul)
    ref = oracle.bilinear_f64(x, h, w, mul)
    ulp = _ulp_of_max(ref)
    e_k = float((got.double() - ref).abs().max()) / ulp
    e_t = float(((F.interpolate(x, (h, w), mode="bilinear") * mul).double() - ref).abs().max()) / ulp
    differ = float((got != want).float().mean())
    _report("resize", "%s %s mul %g" % (name, _rs(shape), mul), differ=differ, kernel_ulp=e_k, torch_ulp=e_t, tol_ulp=RESIZE_DEF_ULP)
    assert torch.equal(got, want), differ
    assert e_t <= RESIZE_TORCH_ULP, e_t                         # torch's own figure, on which the kernel's allowance rests, still holds
    assert e_k <= RESIZE_DEF_ULP, e_k


@pytest.mark.parametrize("mul", [255.0, 1.0])
@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=_rs)
def test_resize_exact_and_definition_fp64(backend, oracle, shape, mul):
    ops, dev, name = backend
    _resize_checks(ops, dev, name, oracle, shape, mul)


@pytest.mark.gpu
@pytest.mark.parametrize("mul", [255.0, 1.0])
def test_resize_540p_non_integer_ratio(hip_ops, oracle, mul):
    ops, dev = hip_ops
    _resize_checks(ops, dev, "hip", oracle, ((540, 960), (181, 320)), mul)


# ---------------------------------------------------------------------------------------------------------------------
# 3. equalize_prepare: uint8 truncation, histogram, torchvision's equalisation LUT.
# Inputs stay in [0, 256): outside it x.to(torch.uint8) is undefined in torch and the kernel's clamp to 0 / 255 is its own choice,
# so nothing out of range is compared with torch.
# ---------------------------------------------------------------------------------------------------------------------
def _eq_input(kind, C, h, w):
    g = torch.Generator().manual_seed(len(kind) * 100 + h + w)
    r = torch.rand(1, C, h, w, generator=g)
    if kind == "uniform":
        return r * 255.999                                      # bin 255 occupied: last == 255
    if kind == "dark":
        return r ** 4 * 40                                      # few bins, large step
    if kind == "two":
        return (r > 0.9).float() * 200 + 7                      # two occupied bins
    if kind == "top":
        return 255 - r ** 3 * 30                                # everything in the top bins
    if kind in ("zero", "full"):
        return torch.full((1, C, h, w), 0.0 if kind == "zero" else 255.0)       # one bin: step == 0, identity, at both ends
    if kind == "sparse":
        x = torch.full((1, C, h * w), 250.0)                    # 200 < 255 pixels outside the last occupied bin: step == 0 with two bins
        x[:, :, torch.randperm(h * w, generator=g)[:200]] = 3.0
        return x.view(1, C, h, w)
    assert kind == "border"                                     # truncation, not rounding: k and k + 0.99999 land in bin k; -0.0 in 0
    ks = torch.tensor([0.0, 1.0, 2.0, 7.0, 127.0, 128.0, 200.0, 254.0, 255.0])
    vals = torch.cat([ks, ks + 0.99999, torch.tensor([-0.0, 0.5, 254.5])])
    assert float(vals.max()) < 256.0
    return vals[torch.randint(0, len(vals), (1, C, h, w), generator=g)]


def _lut_ref(q8):
    """_scale_channel's table itself (oracle.equalize_channel_u8 only applies it); the identity when step == 0"""
    hist = torch.bincount(q8.reshape(-1).long(), minlength=256)
    nz = hist[hist != 0]
    step = int(nz[:-1].sum()) // 255
    if step == 0:
        return torch.arange(256, dtype=torch.int32)
    lut = (torch.cumsum(hist, 0) + step // 2) // step
    return torch.cat([lut.new_zeros(1), lut[:-1]]).clamp(0, 255).to(torch.int32)


def _equalize_checks(ops, dev, name, oracle, kind, C, h, w):
    x = _eq_input(kind, C, h, w)
    n = h * w
    bq = torch.full((C * n + TAIL,), 111, dtype=torch.uint8, device=dev)
    q = bq[:C * n]
    bh, hist = _guarded(C * 256, torch.int32, dev)
    bl, lut = _guarded(C * 256, torch.int32, dev)
    ops.lib.call("zt_equalize_prepare_u8", x.to(dev), q, hist, lut, C, n, _stream(dev))
    assert bool((bq[C * n:] == 111).all()) and _untouched(bh, C * 256) and _untouched(bl, C * 256)
    q, hist, lut = q.view(C, n).cpu(), hist.view(C, 256).cpu(), lut.view(C, 256).cpu()
    q8 = x[0].to(torch.uint8).view(C, n)
    ref_hist = torch.stack([torch.bincount(q8[c].long(), minlength=256) for c in range(C)])
    ref_lut = torch.stack([_lut_ref(q8[c]) for c in range(C)])
    applied = torch.gather(lut.long(), 1, q.long()).to(torch.uint8).view(C, h, w)
    _report("equalize", "%s %s c%d %dx%d" % (name, kind, C, h, w), bins=int((ref_hist[0] != 0).sum()), max_count=int(ref_hist.max()),
            identity=int(torch.equal(ref_lut[0], torch.arange(256, dtype=torch.int32))))
    assert torch.equal(q, q8)
    assert torch.equal(hist.long(), ref_hist) and int(hist.sum()) == C * n
    assert torch.equal(applied, oracle.equalize_u8(q8.view(C, h, w)))
    assert torch.equal(lut, ref_lut)                            # the bins no pixel uses as well
    q2, hist2, lut2 = ops.equalize_prepare(x.to(dev))           # the wrapper the plan calls
    assert torch.equal(q2.cpu(), q) and torch.equal(hist2.cpu(), hist) and torch.equal(lut2.cpu(), lut)


EQ_KINDS = ["uniform", "dark", "two", "top", "zero", "full", "sparse", "border"]


@pytest.mark.parametrize("kind", EQ_KINDS)
def test_equalize_prepare_branches(backend, oracle, kind):
    ops, dev, name = backend
    _equalize_checks(ops, dev, name, oracle, kind, 3, 37, 53)


# 1 channel (C is a parameter); 7 x 9 = 63 pixels, less than one 256-lane block; 300 x 400 = 120 000 pixels over ceil(hw / 2048) = 59
# workgroups of 256 lanes: the grid-stride loop runs eight times per workgroup
@pytest.mark.parametrize("kind,C,h,w", [("uniform", 1, 37, 53), ("dark", 1, 7, 9), ("uniform", 3, 7, 9), ("dark", 3, 300, 400)],
                         ids=lambda v: str(v))
def test_equalize_prepare_sizes(backend, oracle, kind, C, h, w):
    ops, dev, name = backend
    _equalize_checks(ops, dev, name, oracle, kind, C, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "two"])
def test_equalize_prepare_1080p(hip_ops, oracle, kind):
    """2 073 600 pixels per channel over the capped grid of 256 workgroups; "two" puts 1.87 M of them into one bin"""
    ops, dev = hip_ops
    _equalize_checks(ops, dev, "hip", oracle, kind, 3, 1080, 1920)


# ---------------------------------------------------------------------------------------------------------------------
# 4. raft_pack_input / zt_raft_pack_pair: raft.py's InputPadder (centred replicate padding to a multiple of 8) and 2 (x / 255) - 1
# into the stem's NHWC layout: 3 channels and ld - 3 zeros per pixel.  (40,56) pads by 0, (37,53) by 3 = 1 + 2 on each axis,
# (33,49) by 7 = 3 + 4, (8,8) is one 8 x 8 block.
# ---------------------------------------------------------------------------------------------------------------------
PACK_SIZES = [(40, 56), (37, 53), (33, 49), (8, 8)]


def _pack_ref(x255, Hp, Wp):
    h, w = x255.shape[-2:]
    ph, pw = Hp - h, Wp - w
    y = F.pad(2 * (x255 / 255.0) - 1.0, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], mode="replicate")
    return y[0].permute(1, 2, 0).contiguous()                   # [Hp, Wp, 3]


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", PACK_SIZES, ids=lambda s: "%dx%d" % s)
def test_raft_pack_padding_and_zero_channels(backend, oracle, hw, dt):
    ops, dev, name = backend
    h, w = hw
    Hp, Wp = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    assert (Hp, Wp) == ((((h // 8) + 1) * 8 - h) % 8 + h, (((w // 8) + 1) * 8 - w) % 8 + w)     # raft.py's own formula
    adt, ld = (torch.bfloat16, 8) if dt else (torch.float32, 4)
    g = torch.Generator().manual_seed(h * 64 + w)
    a = torch.rand(1, 3, h, w, generator=g) * 255.0             # frame 1: the resized cache * 255, not quantised
    b = torch.rand(1, 3, h, w, generator=g) ** 2 * 180.0        # frame 2: goes through the truncation and the LUT of section 3
    q2, _, lut = ops.equalize_prepare(b.to(dev))
    b_eq = oracle.equalize_u8(b[0].to(torch.uint8)).float()[None]
    if h * w > 1000:                                            # (8 x 8: fewer than 255 pixels, step == 0, the identity)
        assert not torch.equal(b_eq, b[0].to(torch.uint8).float()[None])
    n = 2 * Hp * Wp * ld
    buf, out = _guarded(n, adt, dev, head=TAIL)
    ops.lib.call("zt_raft_pack_input", a.to(dev), q2, lut, out, dt, ld, h, w, Hp, Wp, _stream(dev))
    assert _untouched(buf, n, head=TAIL)
    out = out.view(2, Hp, Wp, ld)
    via_ops = ops.raft_pack_input(a.to(dev), q2, lut, h, w, dtype=adt)
    assert tuple(via_ops.shape) == (2, Hp, Wp, ld) and torch.equal(via_ops, out)
    ref = torch.stack([_pack_ref(a, Hp, Wp), _pack_ref(b_eq, Hp, Wp)]).to(adt)
    got = out.cpu()
    _report("pack-input", "%s %dx%d->%dx%d dt%d" % (name, h, w, Hp, Wp, dt), differ=float((got[..., :3] != ref).float().mean()))
    assert torch.equal(got[..., :3], ref)                       # fp32: the same three operations; bf16: one rounding of them
    assert bool((got[..., 3:] == 0).all())                      # the stem multiplies these slots by zero weights but sums them
    # two float frames through zt_raft_pack_pair with Hp > h and Wp > w
    bufp, outp = _guarded(n, adt, dev, head=TAIL)
    ops.lib.call("zt_raft_pack_pair", a.to(dev), b.to(dev), outp, dt, ld, h, w, Hp, Wp, _stream(dev))
    assert _untouched(bufp, n, head=TAIL)
    outp = outp.view(2, Hp, Wp, ld)
    refp = torch.stack([_pack_ref(a, Hp, Wp), _pack_ref(b, Hp, Wp)]).to(adt)
    assert torch.equal(outp.cpu()[..., :3], refp) and bool((outp[..., 3:] == 0).all())
    assert torch.equal(outp[0], out[0])                         # frame 1 of the pair == raft_pack_input's first frame of image 1
    assert torch.equal(outp[1], ops.raft_pack_input(b.to(dev), q2, lut, h, w, dtype=adt)[0])    # ... and of image 2


# ---------------------------------------------------------------------------------------------------------------------
# 5. the 7x7 stride-2 stem.  Output tiles are 4 rows x 32 columns: (1,8,8) is one partial tile, (2,23,77) -> 12 x 39 is odd on both
# axes with two tiles in x, (1,9,131) -> 5 x 66 has three tiles in x with two columns in the last, (1,16,136) -> 8 x 68, (2,24,40) -> 12 x 20.
# ---------------------------------------------------------------------------------------------------------------------
STEM_SHAPES = [(1, 8, 8), (2, 23, 77), (1, 9, 131), (1, 16, 136), (2, 24, 40)]


def _nhwc8(x):
    """[N,3,H,W] fp32 (bf16-representable) -> the stem's input: NHWC bf16, 8 channels, 3..7 zero"""
    N, _, H, W = x.shape
    out = torch.zeros(N, H, W, 8, dtype=torch.bfloat16)
    out[..., :3] = x.permute(0, 2, 3, 1).bfloat16()
    return out


def _stem(ops, dev, xd, wd, bd, Ho, Wo, relu):
    N, H, W, _ = xd.shape
    n = N * Ho * Wo * 64
    buf, out = _guarded(n, torch.bfloat16, dev, head=TAIL)
    ops.lib.call("zt_raft_stem_conv_bf16", xd, N, H, W, wd, bd, out, 64, int(relu), _stream(dev))
    assert _untouched(buf, n, head=TAIL)
    via_ops = ops.raft_stem_bf16(xd, wd, bd, relu=relu)
    assert tuple(via_ops.shape) == (N, Ho, Wo, 64) and torch.equal(via_ops.view(-1), out)
    return out.view(N, Ho, Wo, 64)


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_stem_shapes(backend, shape):
    ops, dev, name = backend
    N, H, W = shape
    g = torch.Generator().manual_seed(H * 200 + W)
    x = torch.randn(N, 3, H, W, generator=g).bfloat16().float()
    w = torch.randn(64, 3, 7, 7, generator=g) / 12.0
    b = torch.randn(64, generator=g) * 0.1
    ref = F.conv2d(x.double(), w.bfloat16().double(), b.double(), stride=2, padding=3)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert tuple(ref.shape) == (N, 64, Ho, Wo)
    xd, wd, bd = _nhwc8(x).to(dev), ops.raft_stem_weight_bf16(w.to(dev)), b.to(dev)
    y = _stem(ops, dev, xd, wd, bd, Ho, Wo, False)
    e = _excess(y.cpu().permute(0, 3, 1, 2), ref)
    _report("stem", "%s %dx%dx%d" % (name, N, H, W), excess=e, abs=float((y.cpu().permute(0, 3, 1, 2).double() - ref).abs().max()), tol=BF16_TOL)
    assert e < BF16_TOL, e
    yr = _stem(ops, dev, xd, wd, bd, Ho, Wo, True)
    assert torch.equal(yr, torch.relu(y)) and bool((yr == 0).any()) and bool((yr > 0).any())


def test_stem_weight_repack_and_single_column(backend):
    """k = kx * 8 + c: the repacked tensor against the permutation written in torch, then weights of magnitude 100 in ONE kernel
    column kx and zeros elsewhere -- a column read one pixel off changes every output by the size of the output itself"""
    ops, dev, name = backend
    g = torch.Generator().manual_seed(57)
    w = torch.randn(64, 3, 7, 7, generator=g)
    want = torch.zeros(7, 64, 8, 8)                             # [ky][cout][kx (7 + one padding)][c (3 + 5 padding)]
    want[:, :, :7, :3] = w.permute(2, 0, 3, 1)                  # [ky][cout][kx][c]
    got = ops.raft_stem_weight_bf16(w.to(dev))
    assert tuple(got.shape) == (7, 64, 64) and torch.equal(got.cpu(), want.view(7, 64, 64).bfloat16())
    N, H, W = 1, 10, 21
    x = torch.randn(N, 3, H, W, generator=g).bfloat16().float()
    b = torch.randn(64, generator=g) * 0.1
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for kx in range(7):
        w1 = torch.zeros(64, 3, 7, 7)
        w1[:, :, :, kx] = 100.0 * torch.randn(64, 3, 7, generator=g)
        ref = F.conv2d(x.double(), w1.bfloat16().double(), b.double(), stride=2, padding=3)
        y = _stem(ops, dev, _nhwc8(x).to(dev), ops.raft_stem_weight_bf16(w1.to(dev)), b.to(dev), Ho, Wo, False)
        e = _excess(y.cpu().permute(0, 3, 1, 2), ref)
        _report("stem-column", "%s kx %d" % (name, kx), excess=e, ref_max=float(ref.abs().max()), tol=BF16_TOL)
        # |ref| reaches 2e3 here; the contract's |ref| 2^-8 term is the one bf16 rounding of the result, and what is left for the fp32
        # accumulation of 21 products is the same 2e-3 as everywhere (measured excess: negative on the emulator and on the MI355X)
        assert e < BF16_TOL, (kx, e)


# ---------------------------------------------------------------------------------------------------------------------
# 6. fused correlation volume + pyramid (zt_corr.hip): 64 source pixels x (8 rows x 32 columns) of image 2 per workgroup.
# 16 x 16 is the smallest map the entry point takes (two row bands, half a column tile), 17 x 19 is odd on both axes
# (npx = 323: ragged source tile, level-0 rows 4 bytes off the 16-byte grid, every level drops a row or column), 16 x 33 spills one
# column into a second column tile (and 33 is odd).
# ---------------------------------------------------------------------------------------------------------------------
CORR_SIZES = [(16, 16), (17, 19), (16, 33)]


def _corr_launch(ops, dev, f1, f2, h, w, extra):
    """-> corr0 [npx, ld0] and the three levels, every buffer guarded; ld0 = the wrapper's pitch + extra padding columns"""
    npx = h * w
    ld0 = (npx + 3) // 4 * 4 + extra
    dims = [(h >> l, w >> l) for l in (1, 2, 3)]
    b0, c0 = _guarded(npx * ld0, torch.float32, dev)
    lv = [_guarded(npx * a * b, torch.float32, dev) for a, b in dims]
    ops.lib.call("zt_corr_volume_pyramid_bf16", f1, f1.shape[-1], f2, f2.shape[-1], h, w, 1.0 / 16.0, c0, ld0, lv[0][1], lv[1][1], lv[2][1],
                 _stream(dev))
    assert _untouched(b0, npx * ld0) and all(_untouched(b, npx * a * bb) for (b, _), (a, bb) in zip(lv, dims))
    c0 = c0.view(npx, ld0)
    # ops.corr_volume_pyramid_bf16 hands out corr0 from torch.empty and documents that the launch does not write columns
    # npx .. ld0 - 1: they must still hold the sentinel, not zero
    assert bool((c0[:, npx:] == SENT).all())
    return c0, [v.view(npx, a, b) for (_, v), (a, b) in zip(lv, dims)]


def _corr_checks(ops, dev, name, h, w, structured):
    npx = h * w
    if structured:
        # f1 row i one-hot in channel i % 256; f2 row j one-hot in channel j % 256 with the value 1 + j % 251 (the pixel index itself is not
        # a bf16 number past 256; 251 is prime, so the value pattern never lines up with the channel pattern): entry (i, j) is exactly
        # (1 + j % 251) / 16 where i = j mod 256 and exactly 0 elsewhere, and every pooled level is an exact fp32 number too
        idx = torch.arange(npx)
        f1 = torch.zeros(npx, 256)
        f1[idx, idx % 256] = 1.0
        f2 = torch.zeros(npx, 256)
        f2[idx, idx % 256] = 1.0 + (idx % 251).float()
    else:
        g = torch.Generator().manual_seed(h * 1000 + w)
        f1, f2 = torch.randn(npx, 256, generator=g), torch.randn(npx, 256, generator=g)
    f1, f2 = f1.bfloat16(), f2.bfloat16()
    ref = (f1.double() @ f2.double().t()) / 16.0                # [npx1][npx2]
    tol = 0.0 if structured else 2e-5 * float(ref.abs().max())
    c0, levels = _corr_launch(ops, dev, f1.to(dev), f2.to(dev), h, w, 4)
    errs = [float((c0[:, :npx].cpu().double() - ref).abs().max())]
    lvl = ref.view(npx, 1, h, w)
    for got in levels:
        lvl = F.avg_pool2d(lvl, 2, stride=2)
        assert tuple(got.shape) == (npx, lvl.shape[2], lvl.shape[3])
        errs.append(float((got.cpu().double() - lvl[:, 0]).abs().max()))
    _report("corr-fused", "%s %dx%d %s" % (name, h, w, "one-hot" if structured else "random"), l0=errs[0], l1=errs[1], l2=errs[2], l3=errs[3], tol=tol)
    assert all(e <= tol for e in errs), errs
    # the wrapper: its own pitch, the same numbers
    corr0, lv2 = ops.corr_volume_pyramid_bf16(f1.to(dev), f2.to(dev), h, w, 1.0 / 16.0)
    assert tuple(corr0.shape) == (1, h, w, (npx + 3) // 4 * 4)
    assert torch.equal(corr0.view(npx, -1)[:, :npx], c0[:, :npx]) and all(torch.equal(a, b) for a, b in zip(lv2, levels))
    # the stand-alone pyramid of the fused level 0.  Both pool each level from the ROUNDED level below (as fmap_pyramid does), but not
    # in the same order: corr_pool sums ((a + b) + c) + d, the fused kernel (a + b) + (c + d), so they are not equal bit for bit.
    # One pooling step of either order is within 2 u S of the exact sum S' of its four inputs (u = 2^-24, S = sum of |inputs|; three
    # additions, each rounding a partial sum no larger than S), hence the two are within 4 u S / 4 = 4 u mean|inputs| of each other
    # after the exact * 0.25; a difference at level L - 1 passes through the average undiminished at most.  By induction
    # |fused_L - chain_L| <= 4 L u avgpool^L(|corr0|) (1 + O(u)); a 1 % margin covers the O(u) terms.
    chain = ops.corr_pyramid(corr0, h, w)
    mag = c0[:, :npx].cpu().double().abs().view(npx, 1, h, w)
    worst = 0.0
    for L, (a, b) in enumerate(zip(levels, chain), 1):
        mag = F.avg_pool2d(mag, 2, stride=2)
        bound = 4 * L * 2.0 ** -24 * 1.01 * mag[:, 0]
        d = (a.cpu().double() - b.cpu().double()).abs()
        worst = max(worst, float((d / bound.clamp(min=1e-300)).max()))
        assert bool((d <= bound).all()), L
    _report("corr-fused-vs-pool", "%s %dx%d" % (name, h, w), worst_over_bound=worst)
    if structured:
        assert all(torch.equal(a, b) for a, b in zip(levels, chain))                # exact sums have no order


@pytest.mark.parametrize("structured", [False, True], ids=["random", "one-hot"])
@pytest.mark.parametrize("h,w", CORR_SIZES, ids=lambda v: str(v))
def test_corr_volume_pyramid_small_maps(backend, h, w, structured):
    ops, dev, name = backend
    _corr_checks(ops, dev, name, h, w, structured)


@pytest.mark.gpu
@pytest.mark.parametrize("structured", [False, True], ids=["random", "one-hot"])
def test_corr_volume_pyramid_46x62(hip_ops, structured):
    """six row bands, two column tiles with 30 columns in the second, 45 source tiles with 36 pixels in the last; 46 -> 23 -> 11 -> 5"""
    ops, dev = hip_ops
    _corr_checks(ops, dev, "hip", 46, 62, structured)


# ---------------------------------------------------------------------------------------------------------------------
# 7. warp.  zt_warp2_f32 runs warp2_tiled_kernel for 3-channel images whose flow window fits 68 x 12 per 64 x 8 tile
# (int(64 Wf / W) + 3 <= 68 and int(8 Hf / H) + 3 <= 12), else warp2_kernel.  Cases (H, W, Hf, Wf):
#   (16,128,19,131): int(65.5) + 3 = 68 and int(9.5) + 3 = 12, both at the cap -> tiled; (19,131,23,135): 65 + 3, 9 + 3 -> tiled, and
#   its second column tile stages 67 flow columns (130 + 1 - 65 + 1), the widest window the bound lets through: 64 Wf / W < 66 means
#   the tile's first and last source coordinates are less than 64.97 apart, so i0 .. i1 spans at most 65 + 2 columns, one below the 68
#   of WARP_FWW (a window of 66 columns in LDS fails this case on the emulator, one of 67 is enough for every admitted shape);
#   (16,128,20,131): 10 + 3 = 13 > 12; (16,128,19,132): 66 + 3 = 69 > 68; (16,128,20,132): both -> the plain kernel;
#   (136,168,136,168) full-resolution flow (the copy branch); (24,136,8,46) a padded 1/3-resolution flow; (129,131,43,44);
#   (24,136,1,1), (24,136,3,17), (24,136,24,17) (one axis at full resolution: the fma branch with weights 1 and 0), (3,2,1,1) the
#   smallest image the entry point takes, (13,200,16,200);
#   (9,70,16,72), (20,66,40,136), (17,65,6,22): narrow images, where torch is no reference for the up-sampled coordinates.
# ---------------------------------------------------------------------------------------------------------------------
WARP_CASES = [(16, 128, 19, 131), (19, 131, 23, 135), (16, 128, 20, 131), (16, 128, 19, 132), (16, 128, 20, 132), (136, 168, 136, 168),
              (24, 136, 8, 46), (129, 131, 43, 44), (24, 136, 1, 1), (24, 136, 3, 17), (24, 136, 24, 17), (3, 2, 1, 1), (13, 200, 16, 200),
              (9, 70, 16, 72), (20, 66, 40, 136), (17, 65, 6, 22)]
# Covering condition (a test of zeros must not pass, nor one of interior pixels alone): at amplitude 2 at least half the pixels have all
# four taps inside the image; at amplitude 40 at least 5 % have, and at least 5 % have a tap outside.  Not held to it, because their
# geometry samples (almost) nothing or a single point whatever the random flow is: the 1 x 1 flows (every pixel goes to one place), and
# (24,136,3,17) / (24,136,24,17) at amplitude 40.
WARP_NO_COVER = {(3, 2, 1, 1, 2.0), (3, 2, 1, 1, 40.0), (24, 136, 1, 1, 2.0), (24, 136, 1, 1, 40.0), (24, 136, 24, 17, 40.0), (24, 136, 3, 17, 40.0)}
# Three more have a ceiling below those shares that is in the shapes, whatever the seed (over 40 seeds their shares stay within
# 0.075 - 0.115, 0.41 - 0.46 and 0.012 - 0.037).  warp_tensor scales x by H / Hf and y by W / Wf (sic), so
#   (24,136,24,17) amp 2: y is multiplied by 8, only image rows 0..2 of 24 sample inside: share <= 3 / 24;
#   (9,70,16,72) amp 2: the 16 flow rows span y = 0 .. 14.6 over an image of 9 rows: rows 5..8 sample below it: share <= 5 / 9;
#   (17,65,6,22) amp 40: sigma = 40 * W / Wf = 118 px in y against 17 rows.
# They are held to a floor of 1 % instead, and to the 5 % with a tap outside.
WARP_LOW_COVER = {(24, 136, 24, 17, 2.0), (9, 70, 16, 72, 2.0), (17, 65, 6, 22, 40.0)}
# (24,136,8,46) at amplitude 40 sits at the 5 % line (0.046 - 0.076 over the seeds tried): its generator is offset to one that gives 0.073
WARP_SEED_OFFSET = {(24, 136, 8, 46): 1000}
TAP_CLAMP = 2147483000.0                                        # zt_warp.hip clamps the recorded taps here (2147483008 as fp32)


def _warp_launch(ops, dev, flow, imgA, imgB, want_taps=True):
    _, C, H, W = imgA.shape
    Hf, Wf = flow.shape[-2:]
    n = C * H * W
    bA, oA = _guarded(n, torch.float32, dev)
    bB, oB = _guarded(n, torch.float32, dev) if imgB is not None else (None, None)
    bT, tp = _guarded(H * W * 2, torch.int32, dev) if want_taps else (None, None)
    ops.lib.call("zt_warp2_f32", flow.to(dev), Hf, Wf, imgA.to(dev), None if imgB is None else imgB.to(dev), oA, oB, tp, C, H, W, _stream(dev))
    assert _untouched(bA, n) and (bB is None or _untouched(bB, n)) and (bT is None or _untouched(bT, H * W * 2))
    return (oA.view(1, C, H, W).cpu(), None if oB is None else oB.view(1, C, H, W).cpu(), None if tp is None else tp.view(H, W, 2).cpu())


def _clamped_taps(t):
    """fp32 floor(ix), floor(iy) -> what the kernels record: clamped to +- 2147483000 before the conversion"""
    return t.clamp(-TAP_CLAMP, TAP_CLAMP).to(torch.int32)


def _warp_checks(ops, dev, name, oracle, case, amp, nonfinite=None):
    H, W, Hf, Wf = case
    g = torch.Generator().manual_seed(WARP_SEED_OFFSET.get(case, 0) + H * 7 + W * 5 + Hf * 3 + Wf)
    flow = torch.randn(1, 2, Hf, Wf, generator=g) * amp
    if nonfinite is not None:
        flow = nonfinite
    img = torch.rand(1, 4, H, W, generator=g)
    img3 = img[:, :3].contiguous()
    ref, ref_taps, inside = oracle.warp_fma32(flow, img3)
    A, B, taps = _warp_launch(ops, dev, flow, img3, 0.5 * img3)
    A1, _, taps1 = _warp_launch(ops, dev, flow, img3, None)
    A0, B0, _ = _warp_launch(ops, dev, flow, img3, 0.5 * img3, want_taps=False)
    A4, B4, taps4 = _warp_launch(ops, dev, flow, img, 0.5 * img)
    all_in, any_out = float(inside.all(0).float().mean()), float((~inside).any(0).float().mean())
    finite = nonfinite is None
    eq = (lambda a, b: torch.equal(a, b)) if finite else (lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)))
    _report("warp", "%s %dx%d flow %dx%d amp %g" % ((name,) + case + (amp,)), differ=float((A != ref).float().mean()), all_inside=all_in,
            tap_outside=any_out, nan=float(torch.isnan(A).float().mean()))
    assert eq(A, ref)                                                               # (a) values against the restatement
    if finite:
        assert torch.equal(taps, _clamped_taps(ref_taps))                           # (b) taps: the restatement's ...
        if W >= 128 and amp <= 1e7:
            # ... and ATen's, where ATen's coordinates are the same: narrower, they are an ulp off in places and torch is no reference
            # (beyond 1e7 the int32 conversion of oracle.warp_taps is none either)
            assert torch.equal(taps, oracle.warp_taps(flow, H, W)[0])
    assert eq(B, 0.5 * A)                                                           # (c) a power of two commutes with every rounding
    assert eq(A1, A) and torch.equal(taps1, taps)                                   # (d) one image == two images
    assert eq(A0, A) and eq(B0, B)                                                  #     and the taps are optional
    assert eq(A4[:, :3], A) and eq(B4[:, :3], B) and torch.equal(taps4, taps)       # (e) 4 channels take warp2_kernel
    assert eq(A4[:, 3:], oracle.warp_fma32(flow, img[:, 3:].contiguous())[0])
    if W >= 128 and amp <= 1e7:
        assert eq(A, oracle.warp_tensor(flow, img3))
    nowhere = ~inside.any(0)
    if finite:
        assert bool((A[0][:, nowhere] == 0).all())                                  # no tap in the image: exactly zero
    return all_in, any_out


@pytest.mark.parametrize("amp", [2.0, 40.0])
@pytest.mark.parametrize("case", WARP_CASES, ids=lambda c: "%dx%d-f%dx%d" % c)
def test_warp_cases(backend, oracle, case, amp):
    ops, dev, name = backend
    all_in, any_out = _warp_checks(ops, dev, name, oracle, case, amp)
    if case + (amp,) in WARP_NO_COVER:
        return
    if case + (amp,) in WARP_LOW_COVER:
        assert all_in >= 0.01 and any_out >= 0.05, (all_in, any_out)
    elif amp == 2.0:
        assert all_in >= 0.5, all_in
    else:
        assert all_in >= 0.05 and any_out >= 0.05, (all_in, any_out)


@pytest.mark.parametrize("amp", [300.0, 1e7, 1e12])
def test_warp_flow_leaves_the_image(backend, oracle, amp):
    """21 x 130 under an 8 x 48 flow: most coordinates land far outside.  At 1e7 the coordinates reach about 3e7 px, still below the
    clamp of the recorded taps (2147483000); 1e12 is added so that the clamp itself is compared"""
    ops, dev, name = backend
    H, W, Hf, Wf = case = (21, 130, 8, 48)
    _, any_out = _warp_checks(ops, dev, name, oracle, case, amp)
    assert any_out >= 0.9
    # the clamped reference from torch's own coordinates (W >= 128: the same bits as the restatement's)
    g = torch.Generator().manual_seed(H * 7 + W * 5 + Hf * 3 + Wf)
    flow = torch.randn(1, 2, Hf, Wf, generator=g) * amp
    grid = oracle.warp_coords(flow, H, W)[0]
    ix = oracle._fma32(grid[..., 0] + 1, torch.tensor(W / 2.0, dtype=torch.float32), torch.tensor(-0.5))
    iy = oracle._fma32(grid[..., 1] + 1, torch.tensor(H / 2.0, dtype=torch.float32), torch.tensor(-0.5))
    want = _clamped_taps(torch.stack([torch.floor(ix), torch.floor(iy)], -1))
    _, _, taps = _warp_launch(ops, dev, flow, torch.zeros(1, 3, H, W), None)
    on_clamp = float((want.abs() == 2147483008).any(-1).float().mean())
    _report("warp-leaving", "%s amp %g" % (name, amp), taps_on_clamp=on_clamp)
    assert torch.equal(taps, want)
    assert on_clamp > 0.5 if amp == 1e12 else on_clamp == 0.0


def test_warp_non_finite_flow(backend, oracle):
    """inf, -inf, NaN and 3e38 in an otherwise zero 8 x 46 flow under a 24 x 136 image: the kernels' fminf / fmaxf clamps turn them
    into far-outside taps whose weights are NaN, so the same pixels are NaN as in torch's grid_sample and all others are equal;
    only clamped addresses are read, and nothing is written outside the outputs (checked by every launch of _warp_checks)"""
    ops, dev, name = backend
    flow = torch.zeros(1, 2, 8, 46)
    flow[0, 0, 1, 5], flow[0, 1, 2, 20], flow[0, 0, 5, 30], flow[0, 1, 6, 40] = float("inf"), float("-inf"), float("nan"), 3e38
    H, W = 24, 136
    _warp_checks(ops, dev, name, oracle, (H, W, 8, 46), 0.0, nonfinite=flow)
    img = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(3))
    A, _, _ = _warp_launch(ops, dev, flow, img, None)
    ref = oracle.warp_tensor(flow, img)
    nan = torch.isnan(ref)
    _report("warp-non-finite", name, nan=float(nan.float().mean()))
    assert 0.0 < float(nan.float().mean()) < 0.5
    assert torch.equal(torch.isnan(A), nan) and torch.equal(A.nan_to_num(7.0), ref.nan_to_num(7.0))
