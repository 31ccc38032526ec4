"""The RAFT refinement loop (RaftPlan.refine_step / finish), one launch at a time against plain torch in fp64.

Covers what the loop's end-to-end goldens only see from a distance: the fused SepConvGRU / residual epilogues of the tiled
convolution (epi 4 / 5 / 6, staged 16-byte path and scalar fallback, 16- and 32-pixel tiles), their fp32 twins, the stand-alone
point-wise GRU kernels, the correlation pyramid and lookup at odd map sizes (fp32 and bf16 output, padded level-0 pitch), the
lookup with the folded flow bookkeeping, and the convex up-sampling.

Every output buffer is pre-filled with a sentinel so that a region a launch must not write can be checked.  bf16 kernels are
held to the project's bf16 contract (test_conv_bf16): max(|got - ref| - |ref| * 2^-8) < 2e-3 with the fp64 reference evaluated
on the bf16-rounded operands.  Each test prints the figure it measured ("RAFTLOOP ..." lines, visible with -s) before it asserts.

Schedule classes (conv2d_bf16_impl in zt_conv.hip, launch_conv_h in zt_conv_tiled.hip), TH = 4 output rows per workgroup:
  c16 = ceil(Cout / 16); NT = 4 when c16 % 4 == 0, 3 when c16 % 3 == 0; MT = 2 (32-pixel tiles) when
  ceil(W / 32) * ceil(H / 4) * ceil(c16 / NT) >= 512, else MT = 1; every stride-1 NT = 4 becomes NT = 2;
  chunk = 64 channels when Cin % 64 == 0 and (taps * NT * 16 + halo pixels) * 160 bytes <= 64 KiB, else 32 channels;
  PD = 2 (two chunks of loads in flight) when MT = 1, Cin > 64 and the grid has at most 1024 workgroups."""
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

SENT = -768.0            # exact in bf16 and fp32; no kernel under test produces it
BF16_TOL = 2e-3          # test_conv_bf16's contract: max(|got - ref| - |ref| * 2^-8) < 2e-3


def _mods():
    return import_module("zero-tig_amd.ops").CV, import_module("zero-tig_amd.lib").current_stream


def _sent(shape, dtype, dev):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


def _is_sent(t):
    return bool((t == SENT).all())


def _excess(got, ref):
    """the bf16 contract's left-hand side"""
    return float(((got.double() - ref).abs() - ref.abs() * 2.0 ** -8).max())


def _maxabs(got, ref):
    return float((got.double() - ref).abs().max())


def _report(what, name, **figs):
    print("RAFTLOOP %s [%s] %s" % (what, name, " ".join("%s=%.3g" % kv for kv in figs.items())))


def _conv_ref(x, w, b, pad):
    """'same' stride-1 convolution in fp64 as one matrix product per tap.  x: nhwc [1,H,W,Cin], w: torch layout [Cout,Cin,KH,KW]."""
    KH, KW = w.shape[2:]
    H, W = x.shape[1:3]
    xp = F.pad(x, (0, 0, pad[1], pad[1], pad[0], pad[0]))
    out = b.view(1, 1, 1, -1).expand(1, H, W, -1).clone() if b is not None else torch.zeros(1, H, W, w.shape[0], dtype=x.dtype, device=x.device)
    for ky in range(KH):
        for kx in range(KW):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    return out


def _bf16_ulps(a, b):
    """largest distance between two bf16 tensors in units in the last place (sign-magnitude bits -> monotonic integers)"""
    def key(t):
        i = t.contiguous().view(torch.int16).int()
        mag = i & 0x7FFF
        return torch.where(i < 0, -mag, mag)
    return int((key(a) - key(b)).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 3. SepConvGRU epilogues: [z | r] = sigmoid(conv), r * h to a second destination (epi 4); h = (1 - z) h + z tanh(conv)
# in place (epi 5).  Operands laid out as RaftPlan._prepare / refine_step do.
# ---------------------------------------------------------------------------------------------------------------------
GRU_GEO = {"1x5": ((1, 5), (0, 2)), "5x1": ((5, 1), (2, 0))}


class _Gru:
    """one GRU half at H x W: the [net | inp | motion | flow] buffer, the packed weights, and the fp64 operands"""

    def __init__(self, ops, dev, H, W, geo, bf16):
        (kh, kw), self.pad = GRU_GEO[geo]
        self.k, self.H, self.W, self.bf16, self.ops, self.dev = (kh, kw), H, W, bf16, ops, dev
        self.adt = torch.bfloat16 if bf16 else torch.float32
        g = torch.Generator().manual_seed(1000 * H + 10 * W + kh)
        hx = torch.cat([torch.tanh(torch.randn(1, H, W, 128, generator=g)), torch.relu(torch.randn(1, H, W, 128, generator=g)),
                        torch.randn(1, H, W, 128, generator=g)], -1)
        s = 2.0 * (384 * kh * kw) ** -0.5                      # pre-activations ~ N(0, 1.5): both the linear part and the tails
        wz, wr, wq = (torch.randn(128, 384, kh, kw, generator=g) * s for _ in range(3))
        bz, br, bq = (torch.randn(128, generator=g) * 0.1 for _ in range(3))
        self.HX0 = hx.to(self.adt).to(dev)                     # never written: every launch works on a clone
        rnd = (lambda t: t.bfloat16().double()) if bf16 else (lambda t: t.double())
        self.wzr64, self.wq64 = rnd(torch.cat([wz, wr])).to(dev), rnd(wq).to(dev)
        self.bzr64, self.bq64 = torch.cat([bz, br]).double().to(dev), bq.double().to(dev)
        self.bzr, self.bq = torch.cat([bz, br]).contiguous().to(dev), bq.to(dev)
        wz, wr, wq = wz.to(dev), wr.to(dev), wq.to(dev)
        if bf16:
            self.wzr = torch.zeros((kh * kw, 256, 384), dtype=torch.bfloat16, device=dev)
            ops.repack_weight_bf16(wz, out=self.wzr, co_off=0)
            ops.repack_weight_bf16(wr, out=self.wzr, co_off=128)
            self.wq = ops.repack_weight_bf16(wq)
        else:
            self.wzr = torch.zeros((kh * kw, 384, 256), dtype=torch.float32, device=dev)
            ops.repack_weight(wz, ldw=256, co_off=0, out=self.wzr)
            ops.repack_weight(wr, ldw=256, co_off=128, out=self.wzr)
            self.wq = ops.repack_weight(wq)

    def conv(self, x, wd, b, cout, **kw):
        kh, kw_ = self.k
        if self.bf16:
            return self.ops.conv2d_bf16(x, wd, b, cout, kh, kw_, self.pad, **kw)
        return self.ops.conv2d(x, wd, b, cout, kh, kw_, 1, self.pad, **kw)

    def launch_zr(self, HX, ZR, RH, off=0):
        """refine_step's zr launch; z goes to channels [off, off + 128) of ZR, r * h to [off, off + 128) of RH"""
        CV, _ = _mods()
        self.conv(HX, self.wzr, self.bzr, 256, act="sigmoid", out=CV(ZR, off, 256), aux=CV(HX, 0, 128), epi=4,
                  out2=CV(RH, off, 128), esplit=128)

    def launch_q(self, RH, HX, ZR, Hbuf, off=0):
        """refine_step's q launch; the state lives in (and is updated in) channels [off, off + 128) of Hbuf"""
        CV, _ = _mods()
        self.conv(CV(RH), self.wq, self.bq, 128, act="tanh", x2=CV(HX, 128, 256), out=CV(Hbuf, off, 128), aux=CV(ZR, 0, 128), epi=5)

    def ref_zr(self):
        c = _conv_ref(self.HX0.double(), self.wzr64, self.bzr64, self.pad)
        return torch.sigmoid(c[..., :128]), torch.sigmoid(c[..., 128:]) * self.HX0[..., :128].double()

    def ref_q(self, z, rh, h):
        """from the STORED z and r * h: one kernel's rounding is not charged to the next"""
        xin = torch.cat([rh.double(), self.HX0[..., 128:].double()], -1)
        q = torch.tanh(_conv_ref(xin, self.wq64, self.bq64, self.pad))
        return (1 - z.double()) * h.double() + z.double() * q


def _gru_pair(ops, dev, name, H, W, geo, bf16, tol, excess):
    G = _Gru(ops, dev, H, W, geo, bf16)
    HX = G.HX0.clone()
    ZR, RH = _sent((1, H, W, 256), G.adt, dev), _sent((1, H, W, 128), G.adt, dev)
    G.launch_zr(HX, ZR, RH)
    z_ref, rh_ref = G.ref_zr()
    ez, er = excess(ZR[..., :128], z_ref), excess(RH, rh_ref)
    az, ar = _maxabs(ZR[..., :128], z_ref), _maxabs(RH, rh_ref)
    assert torch.equal(HX, G.HX0)                               # the zr launch only reads the state
    r_half_untouched = _is_sent(ZR[..., 128:])                  # under epi 4 the r half is never stored
    G.launch_q(RH, HX, ZR, HX)
    h_ref = G.ref_q(ZR[..., :128], RH, G.HX0[..., :128])
    eh, ah = excess(HX[..., :128], h_ref), _maxabs(HX[..., :128], h_ref)
    _report("gru-%s-%s" % ("bf16" if bf16 else "fp32", geo), "%s %dx%d" % (name, H, W), z=ez, rh=er, h=eh, abs_z=az, abs_rh=ar, abs_h=ah, tol=tol)
    assert ez < tol and er < tol, (ez, er)
    assert r_half_untouched
    assert eh < tol, eh
    assert torch.equal(HX[..., 128:], G.HX0[..., 128:])         # the in-place update leaves the x channels it is reading alone


# zr launch: Cout 256, c16 16 -> NT 4 -> 2, 8 cout groups;  q launch: Cout 128, c16 8 -> NT 4 -> 2, 4 cout groups.  Cin 384: 64-channel
# chunks except the 32-pixel 5x1 tile, whose (5 * 32 + 8 * 32) * 160 B = 66 560 B > 64 KiB falls back to 32-channel chunks.
#   5 x 21:   ceil(21/32) * 2 * 4 = 8 < 512 -> MT 1 for both; grids 2 * 8 * 2 = 32 and 2 * 4 * 2 = 16 <= 1024 -> PD 2.  21 = 16 + 5, 5 = 4 + 1
#   9 x 40:   2 * 3 * 4 = 24 -> MT 1; grids 3 * 8 * 3 = 72 and 36 -> PD 2.  40 = 2 * 16 + 8, 9 = 2 * 4 + 1
#   40 x 250: zr 8 * 10 * 4 = 320 < 512 -> MT 1, grid 16 * 8 * 10 = 1280 > 1024 -> PD 1;  q 8 * 10 * 2 = 160 -> MT 1, grid 640 -> PD 2
#   80 x 250: zr 8 * 20 * 4 = 640 >= 512 -> MT 2 (PD 1);  q 8 * 20 * 2 = 320 -> MT 1, grid 16 * 4 * 20 = 1280 -> PD 1
#   129 x 250: zr 8 * 33 * 4 = 1056 -> MT 2;  q 8 * 33 * 2 = 528 >= 512 -> MT 2.  250 = 7 * 32 + 26 and 129 = 32 * 4 + 1: ragged on both axes
GRU_SMALL = [(5, 21), (9, 40)]
GRU_LARGE = [(40, 250), (80, 250), (129, 250)]


@pytest.mark.parametrize("geo", list(GRU_GEO))
@pytest.mark.parametrize("hw", GRU_SMALL, ids=lambda s: "%dx%d" % s)
def test_gru_epilogues_bf16(backend, hw, geo):
    ops, dev, name = backend
    _gru_pair(ops, dev, name, hw[0], hw[1], geo, True, BF16_TOL, _excess)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", list(GRU_GEO))
@pytest.mark.parametrize("hw", GRU_LARGE, ids=lambda s: "%dx%d" % s)
def test_gru_epilogues_bf16_large_tiles(hip_ops, hw, geo):
    ops, dev = hip_ops
    _gru_pair(ops, dev, "hip", hw[0], hw[1], geo, True, BF16_TOL, _excess)


@pytest.mark.parametrize("geo", list(GRU_GEO))
@pytest.mark.parametrize("hw", GRU_SMALL, ids=lambda s: "%dx%d" % s)
def test_gru_epilogues_fp32(backend, hw, geo):
    """fp32 plan (zt_conv2d_nhwc_f32_ex): 2e-5 absolute is test_conv_fwd's figure -- fp32 MFMA accumulation, outputs bounded by 1"""
    ops, dev, name = backend
    _gru_pair(ops, dev, name, hw[0], hw[1], geo, False, 2e-5, _maxabs)


# ---------------------------------------------------------------------------------------------------------------------
# 2. staged 16-byte epilogue against the scalar fallback: the same launch with its outputs at channel offset 8 (16-byte aligned:
# staged path) and 4 (8 bytes off: scalar path) of a wider buffer.  Both meet the fp64 contract and agree bit for bit.
# 9 x 40 -> MT 1 for every case (see above; 3x3 C 64: 2 * 3 * 1 = 6 < 512).
# ---------------------------------------------------------------------------------------------------------------------
def _placed(run, ref):
    """run(off) -> output buffers with the results in channels [off, off + C) and the sentinel elsewhere; ref: their fp64 references"""
    res = {}
    for off in (8, 4):
        bufs = run(off)
        for b, r in zip(bufs, ref):
            e = _excess(b[..., off:off + r.shape[-1]], r)
            _report("placed", "off %d" % off, excess=e, abs=_maxabs(b[..., off:off + r.shape[-1]], r), tol=BF16_TOL)
            assert e < BF16_TOL, (off, e)
            assert _is_sent(b[..., :off]) and _is_sent(b[..., off + r.shape[-1]:])
            res.setdefault(off, []).append((b[..., off:off + r.shape[-1]].contiguous(), e))
    return res


STAGED_CASES = ["epi1", "epi3", "epi6", "epi4-1x5", "epi4-5x1", "epi5-1x5", "epi5-5x1"]


@pytest.mark.parametrize("case", STAGED_CASES)
def test_staged_epilogue_equals_scalar(backend, case):
    ops, dev, name = backend
    CV, _ = _mods()
    H, W = 9, 40
    if case in ("epi1", "epi3", "epi6"):
        epi = int(case[3])
        act = {1: None, 3: "lrelu", 6: "relu"}[epi]
        g = torch.Generator().manual_seed(40 + epi)
        x = torch.randn(1, H, W, 64, generator=g).bfloat16()
        w = torch.randn(64, 64, 3, 3, generator=g) / 24.0
        b = torch.randn(64, generator=g) * 0.1
        aux = torch.randn(1, H, W, 64, generator=g).bfloat16()
        c = _conv_ref(x.double(), w.bfloat16().double(), b.double(), (1, 1))
        a64 = aux.double()
        ref = {1: lambda: c * torch.where(a64 > 0, 1.0, 0.2), 3: lambda: F.leaky_relu(c, 0.2) + a64, 6: lambda: torch.relu(torch.relu(c) + a64)}[epi]()
        xd, auxd, wd, bd = x.to(dev), aux.to(dev), ops.repack_weight_bf16(w.to(dev)), b.to(dev)

        def run(off):
            out = _sent((1, H, W, 80), torch.bfloat16, dev)
            ops.conv2d_bf16(xd, wd, bd, 64, 3, 3, (1, 1), act, out=CV(out, off, 64), aux=auxd, epi=epi, variant=2)
            return [out]
        res = _placed(run, [ref.to(dev)])
    else:
        epi, geo = int(case[3]), case[5:]
        G = _Gru(ops, dev, H, W, geo, True)
        if epi == 4:
            def run(off):
                ZR, RH = _sent((1, H, W, 272), torch.bfloat16, dev), _sent((1, H, W, 144), torch.bfloat16, dev)
                G.launch_zr(G.HX0.clone(), ZR, RH, off)
                return [ZR, RH]                                 # z in [off, off + 128) of ZR: the r half stays on the sentinel
            res = _placed(run, list(G.ref_zr()))
        else:
            g = torch.Generator().manual_seed(77)
            z = torch.sigmoid(torch.randn(1, H, W, 256, generator=g) * 1.5).bfloat16().to(dev)     # [z | unused], ld 256 as in the plan
            rh = (torch.randn(1, H, W, 128, generator=g) * 0.5).bfloat16().to(dev)
            h0 = G.HX0[..., :128]
            ref = G.ref_q(z[..., :128], rh, h0)

            def run(off):
                Hb = _sent((1, H, W, 144), torch.bfloat16, dev)
                Hb[..., off:off + 128] = h0
                HX = G.HX0.clone()
                G.launch_q(rh, HX, z, Hb, off)
                assert torch.equal(HX, G.HX0)
                return [Hb]
            res = _placed(run, [ref])
    for (a, ea), (s, es) in zip(res[8], res[4]):
        ulps = _bf16_ulps(a, s)
        _report("staged-vs-scalar", "%s %s" % (name, case), staged=ea, scalar=es, ulps=ulps, tol=BF16_TOL)
        # both back-ends agree bit for bit (the library is built without floating-point contraction, and both paths round the
        # same fp32 value to bf16 once), so equality is asserted rather than the one-ulp bound
        assert torch.equal(a, s), ulps


# ---------------------------------------------------------------------------------------------------------------------
# 4. ResidualBlock tail of the BatchNorm-folded context encoder: relu(relu(conv3x3 + bias) + residual), epi 6
# ---------------------------------------------------------------------------------------------------------------------
def _res_tail(ops, dev, name, C, H, W):
    g = torch.Generator().manual_seed(C * 7 + H)
    x = torch.randn(1, H, W, C, generator=g).bfloat16()
    res = torch.randn(1, H, W, C, generator=g).bfloat16()
    w = torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    out = _sent((1, H, W, C + 8), torch.bfloat16, dev)
    CV, _ = _mods()
    ops.conv2d_bf16(x.to(dev), ops.repack_weight_bf16(w.to(dev)), b.to(dev), C, 3, 3, (1, 1), "relu", out=CV(out, 0, C), aux=res.to(dev), epi=6)
    ref = torch.relu(res.double().to(dev) + torch.relu(_conv_ref(x.double().to(dev), w.bfloat16().double().to(dev), b.double().to(dev), (1, 1))))
    e = _excess(out[..., :C], ref)
    _report("res-tail-epi6", "%s c%d %dx%d" % (name, C, H, W), excess=e, abs=_maxabs(out[..., :C], ref), tol=BF16_TOL)
    assert e < BF16_TOL, e
    assert _is_sent(out[..., C:])


# C 64: c16 4 -> NT 4 -> 2, 64-channel chunk, Cin <= 64 -> PD 1.   C 96: c16 6 -> NT 3 (the one width with 32-channel chunks:
# 96 % 64 != 0), PD 2.   C 128: c16 8 -> NT 2, 64-channel chunks, PD 2.   All MT 1: ceil(W / 32) * ceil(H / 4) * groups <= 6.
@pytest.mark.parametrize("C,H,W", [(64, 9, 37), (96, 6, 21), (128, 5, 19)], ids=lambda v: str(v))
def test_residual_tail_epi6(backend, C, H, W):
    ops, dev, name = backend
    _res_tail(ops, dev, name, C, H, W)


# 129 x 500: C 64: ceil(500/32) * 33 * 1 = 16 * 33 = 528 >= 512 -> MT 2, NT 2, 32-channel chunks ((9 * 32 + 6 * 34) * 160 B > 64 KiB);
# C 96: 16 * 33 * 2 = 1056 -> MT 2, NT 3, 32-channel chunks.  500 = 15 * 32 + 20, 129 = 32 * 4 + 1.
@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 96])
def test_residual_tail_epi6_large_tiles(hip_ops, C):
    ops, dev = hip_ops
    _res_tail(ops, dev, "hip", C, 129, 500)


# ---------------------------------------------------------------------------------------------------------------------
# 5. stand-alone point-wise GRU kernels (public entry points; the plan's epilogues replace them)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
def test_gru_pointwise(backend, dt):
    ops, dev, name = backend
    _, stream = _mods()
    lib, s = ops.lib, stream(dev)
    adt = torch.bfloat16 if dt else torch.float32
    C, npx = 128, 9 * 40 + 1                                    # 361 * 128 = 180 * 256 + 128: the last 256-lane group is half empty
    g = torch.Generator().manual_seed(5 + dt)
    zr = torch.sigmoid(torch.randn(npx + 1, 256, generator=g) * 1.5).to(adt).to(dev)      # one row more than npx everywhere:
    hx = torch.randn(npx + 1, 384, generator=g).to(adt).to(dev)                           # a launch that runs past the last pixel shows
    q = torch.tanh(torch.randn(npx + 1, 128, generator=g)).to(adt).to(dev)
    zr0, hx0, q0 = zr.clone(), hx.clone(), q.clone()
    rh = _sent((npx + 1, 128), adt, dev)
    lib.call("zt_gru_rh", zr, dt, 256, hx, 384, rh, 128, C, npx, s)
    # bf16: the fp32 product of two bf16 values is exact, so the result is one rounding; fp32: one multiplication
    want = (zr0[:npx, 128:].float() * hx0[:npx, :128].float()).to(adt)
    assert torch.equal(rh[:npx], want)
    assert _is_sent(rh[npx:]) and torch.equal(zr, zr0) and torch.equal(hx, hx0)
    lib.call("zt_gru_update", zr, dt, 256, q, 128, hx, 384, C, npx, s)
    z64, h64, q64 = zr0[:npx, :128].double(), hx0[:npx, :128].double(), q0[:npx].double()
    ref = (1 - z64) * h64 + z64 * q64
    e = _excess(hx[:npx, :128], ref) if dt else _maxabs(hx[:npx, :128], ref)
    tol = BF16_TOL if dt else 1e-6
    _report("gru-update", "%s dt%d" % (name, dt), err=e, abs=_maxabs(hx[:npx, :128], ref), tol=tol)
    assert e < tol, e
    assert torch.equal(hx[:npx, 128:], hx0[:npx, 128:]) and torch.equal(hx[npx:], hx0[npx:])
    assert torch.equal(zr, zr0) and torch.equal(q, q0)


# ---------------------------------------------------------------------------------------------------------------------
# 6 / 7. correlation pyramid and lookup at odd sizes: 17 x 21 -> 8x10 / 4x5 / 2x2, 16 x 19 -> 8x9 / 4x4 / 2x2,
# 23 x 18 -> 11x9 / 5x4 / 2x2: every level drops a row or a column somewhere
# ---------------------------------------------------------------------------------------------------------------------
CORR_MAPS = [(17, 21), (16, 19), (23, 18)]
_corr_cache = {}


def _corr_case(oracle, h, w):
    """computed once per map and shared; nothing in it is ever written"""
    if (h, w) not in _corr_cache:
        g = torch.Generator().manual_seed(h * 100 + w)
        f1, f2 = torch.randn(1, 64, h, w, generator=g), torch.randn(1, 64, h, w, generator=g)
        pyr = oracle.corr_pyramid(f1, f2)
        npx = h * w
        pitch = (npx + 15) // 16 * 16
        c0 = torch.full((1, h, w, pitch), float("nan"))         # level 0 on a padded pitch, NaN in the padding
        c0[0, :, :, :npx] = pyr[0].view(h, w, npx)
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        grid = torch.stack([xs, ys], 0).float()[None]           # [1,2,h,w], (x, y)
        coords = grid + 3.0 * torch.randn(1, 2, h, w, generator=g)
        flat = coords[0].permute(1, 2, 0).reshape(-1, 2)
        planted = [(w - 1.0, h - 1.0), (float(w), float(h)), (-1.0, -1.0), (3.0, 2.0), (-50.0, -50.0), (1e6, 3.0), (-1e9, 1e9)]
        where = [5 + 31 * i for i in range(len(planted))]       # spread over the map (31 * 6 + 5 = 191 < 16 * 19)
        for n, p in zip(where, planted):
            flat[n] = torch.tensor(p)
        coords = flat.view(h, w, 2).permute(2, 0, 1)[None].contiguous()
        look = oracle.corr_lookup(pyr, coords)                  # [1,324,h,w]
        _corr_cache[(h, w)] = dict(pyr=pyr, c0=c0, coords=flat.contiguous(), look=look.permute(0, 2, 3, 1).contiguous(), far=where[4:],
                                   grid=grid[0].permute(1, 2, 0).reshape(-1, 2).contiguous())
    return _corr_cache[(h, w)]


@pytest.mark.parametrize("hw", CORR_MAPS, ids=lambda s: "%dx%d" % s)
def test_corr_pyramid_lookup_odd_sizes(backend, oracle, hw):
    ops, dev, _ = backend
    h, w = hw
    c = _corr_case(oracle, h, w)
    c0 = c["c0"].to(dev)
    levels = ops.corr_pyramid(c0, h, w)
    for lv, ref in zip(levels, c["pyr"][1:]):
        assert tuple(lv.shape[1:]) == tuple(ref.shape[2:])
        assert torch.equal(lv.cpu(), ref[:, 0])                 # bit for bit, and no NaN of the padding pulled in
    coords = c["coords"].to(dev)
    out = _sent((1, h, w, 324), torch.float32, dev)
    ops.corr_lookup(c0, levels, h, w, coords, out=out)
    assert torch.equal(out.cpu(), c["look"])                    # the integer contract of corr.py:29-50 (test_raft_ops_golden) at odd sizes
    far = out.view(h * w, 324)[c["far"]]
    assert far.shape == (3, 324) and bool(torch.isfinite(far).all()) and bool((far == 0).all())
    ob = torch.zeros((1, h, w, 328), dtype=torch.bfloat16, device=dev)
    ops.corr_lookup(c0, levels, h, w, coords, out=ob)
    assert torch.equal(ob[..., :324], out.bfloat16()) and bool((ob[..., 324:] == 0).all())


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", CORR_MAPS, ids=lambda s: "%dx%d" % s)
def test_corr_lookup_step_equals_flow_step_then_lookup(backend, oracle, hw, dt):
    ops, dev, _ = backend
    _, stream = _mods()
    lib, s = ops.lib, stream(dev)
    h, w = hw
    npx = h * w
    c = _corr_case(oracle, h, w)
    c0 = c["c0"].to(dev)
    levels = [p[:, 0].contiguous().to(dev) for p in c["pyr"][1:]]
    adt, ldfin, ldo = (torch.bfloat16, 8, 328) if dt else (torch.float32, 4, 324)
    es = 2 if dt else 4
    g = torch.Generator().manual_seed(npx + dt)
    delta = torch.randn(npx, 4, generator=g)
    delta[:, 2:] = float("nan")                                 # only the first two columns are the flow update
    delta = delta.to(dev)
    coords = c["coords"].to(dev)

    def buffers():
        return dict(F4=_sent((1, h, w, 4), torch.float32, dev), HX=_sent((1, h, w, 384), adt, dev), FIN=_sent((1, h, w, ldfin), adt, dev),
                    CORR=_sent((1, h, w, ldo), adt, dev))
    A, B = buffers(), buffers()
    coordsA = coords.clone()
    lib.call("zt_raft_flow_step", coordsA, delta, 4, h, w, A["F4"], 4, A["HX"].data_ptr() + es * 382, 384, A["FIN"], ldfin, dt, s)
    ops.corr_lookup(c0, levels, h, w, coordsA, out=A["CORR"])
    coordsB = _sent((npx, 2), torch.float32, dev)
    ops.corr_lookup_step(c0, levels, h, w, coords, B["CORR"], delta, coordsB, B["F4"], B["HX"].data_ptr() + es * 382, 384, B["FIN"])
    assert torch.equal(coords.cpu(), c["coords"])               # the fused launch reads its coordinates only
    assert torch.equal(coordsB, coordsA) and torch.equal(coordsB, coords + delta[:, :2])
    flow = coordsB - c["grid"].to(dev)
    for k in ("F4", "HX", "FIN", "CORR"):
        assert torch.equal(A[k], B[k]), k
    assert torch.equal(B["F4"][..., :2].reshape(npx, 2), flow) and _is_sent(B["F4"][..., 2:])
    assert torch.equal(B["HX"][..., 382:].reshape(npx, 2), flow.to(adt)) and _is_sent(B["HX"][..., :382])
    assert torch.equal(B["FIN"][..., :2].reshape(npx, 2), flow.to(adt)) and _is_sent(B["FIN"][..., 2:])
    assert not _is_sent(B["CORR"][..., :324]) and _is_sent(B["CORR"][..., 324:])
    # the looked-up values themselves: the plain lookup at the summed coordinates
    plain = torch.empty((1, h, w, 324), dtype=torch.float32, device=dev)
    ops.corr_lookup(c0, levels, h, w, coordsB, out=plain)
    assert torch.equal(B["CORR"][..., :324], plain.to(adt))


def test_flow_bookkeeping_entry_points(backend, oracle):
    ops, dev, _ = backend
    _, stream = _mods()
    lib, s = ops.lib, stream(dev)
    h, w = 17, 21
    npx = h * w
    c = _corr_case(oracle, h, w)
    grid = c["grid"].to(dev)
    init = _sent((npx + 1, 2), torch.float32, dev)
    lib.call("zt_raft_coords_init_f32", init, h, w, s)
    assert torch.equal(init[:npx], grid) and _is_sent(init[npx:])
    # delta = None: coords1 stays, flow = coords1 - grid
    coords = c["coords"].to(dev)
    c1 = coords.clone()
    F4, FIN = _sent((1, h, w, 4), torch.float32, dev), _sent((1, h, w, 4), torch.float32, dev)
    lib.call("zt_raft_flow_step", c1, None, 0, h, w, F4, 4, None, 0, FIN, 4, 0, s)
    assert torch.equal(c1, coords)
    assert torch.equal(F4[..., :2].reshape(npx, 2), coords - grid) and torch.equal(FIN[..., :2], F4[..., :2])
    assert _is_sent(F4[..., 2:]) and _is_sent(FIN[..., 2:])
    # the fused lookup refuses to alias its two coordinate buffers, and a delta that would not be recorded
    c0 = c["c0"].to(dev)
    levels = [p[:, 0].contiguous().to(dev) for p in c["pyr"][1:]]
    delta = torch.zeros(npx, 4, device=dev)
    for cout in (coords, None):
        out, F4, FIN, HX = (_sent((1, h, w, n), torch.float32, dev) for n in (324, 4, 4, 384))
        with pytest.raises(RuntimeError, match="1001"):
            ops.corr_lookup_step(c0, levels, h, w, coords, out, delta, cout, F4, HX.data_ptr() + 4 * 382, 384, FIN)
        assert all(_is_sent(t) for t in (out, F4, FIN, HX)) and torch.equal(coords.cpu(), c["coords"])


# ---------------------------------------------------------------------------------------------------------------------
# 8. convex 8x up-sampling (raft.py:64-75)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (17, 21)], ids=lambda s: "%dx%d" % s)
def test_convex_upsample(backend, oracle, hw):
    ops, dev, name = backend
    _, stream = _mods()
    lib, s = ops.lib, stream(dev)
    h, w = hw
    g = torch.Generator().manual_seed(h * 31 + w)
    flow = 4.0 * torch.randn(1, h, w, 2, generator=g)
    mask = 3.0 * torch.randn(1, h, w, 576, generator=g)
    F4 = torch.full((1, h, w, 4), float("nan"))
    F4[..., :2] = flow
    F4d, maskd = F4.to(dev), mask.to(dev)
    up, low = _sent((1, 2, 8 * h, 8 * w), torch.float32, dev), _sent((1, 2, h, w), torch.float32, dev)
    lib.call("zt_convex_upsample_f32", F4d, 4, maskd, 576, up, low, h, w, s)
    ref = oracle.convex_upsample(flow.permute(0, 3, 1, 2).double(), mask.permute(0, 3, 1, 2).double())
    # a nine-term convex combination in fp32 whose weights carry a few ulps from expf and the division: about 16 * 2^-24
    # relative to the largest term.  Measured: 1.9e-7 (5 x 7) and 2.6e-7 (17 x 21) relative, the same on the emulator and the MI355X.
    scale = float((8 * flow).abs().max())
    e = _maxabs(up.cpu(), ref)
    _report("convex-upsample", "%s %dx%d" % (name, h, w), err=e, rel=e / scale, tol=2e-6 * scale)
    assert e < 2e-6 * scale, (e, scale)
    assert torch.equal(low.cpu(), flow.permute(0, 3, 1, 2))
    up2 = _sent((1, 2, 8 * h, 8 * w), torch.float32, dev)
    lib.call("zt_convex_upsample_f32", F4d, 4, maskd, 576, up2, None, h, w, s)       # flow_low is optional
    assert torch.equal(up2, up)
    # every logit -1e4: exp(m - max) = 1 for all nine, the weights are exactly uniform (without the max subtraction: 0 / 0).
    # A single non-zero flow vector appears as neighbour k = 0..8 of the nine low-resolution pixels around it, each output
    # is one product weight * 8 * flow plus zeros, so all nine blocks must hold the same bits.
    y0, x0 = h // 2, w // 2
    F1 = torch.zeros(1, h, w, 4)
    F1[0, y0, x0, 0], F1[0, y0, x0, 1] = 3.0, -5.0
    up3 = _sent((1, 2, 8 * h, 8 * w), torch.float32, dev)
    lib.call("zt_convex_upsample_f32", F1.to(dev), 4, torch.full((1, h, w, 576), -1e4, device=dev), 576, up3, None, h, w, s)
    up3 = up3.cpu()
    blocks = up3.view(2, h, 8, w, 8)[:, y0 - 1:y0 + 2, :, x0 - 1:x0 + 2, :]
    for ch, v in ((0, 3.0), (1, -5.0)):
        b = blocks[ch]
        assert bool((b == b[0, 0, 0, 0]).all()), "softmax of equal logits is not uniform"
        assert abs(float(b[0, 0, 0, 0]) - 8.0 * v / 9.0) < 2e-6 * 40.0
    rest = up3.view(2, h, 8, w, 8).clone()
    rest[:, y0 - 1:y0 + 2, :, x0 - 1:x0 + 2, :] = 0
    assert bool((rest == 0).all())
