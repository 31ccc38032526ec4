"""The loss (zt_loss.hip), glue (zt_glue.hip) and optimizer (zt_optim.hip) kernels, one at a time, against plain float64 torch
with gradients from torch.autograd, on inputs that saturate every clamp on purpose.

Tolerance rule (no number is fixed here): every reference is evaluated twice on the same fp32 input values, in float64 and in
float32 torch, and a kernel output may differ from the float64 one by
    max(8 * max|ref32 - ref64|, 4 * 2^-24 * max|ref64|)
where 8 covers another summation order and another libm powf / expf.  The bound is measured on the reference alone.  With
fast_exp = 1 every bilateral weight may be off by 2^-21 relative (v_exp_f32 ~1 ulp plus < 1 ulp from rounding its argument,
|x| < 1), which adds 2^-21 * sum(24 coef) to the ds2 bound and 2^-21 * |term| to the smooth bound.

Guard band: a pre-clamp value within 1e-4 relative of its bound could fall on either side of it in fp32 and in fp64; the input
behind such a value is multiplied by 0.99 until none is left (asserted), and no element is left out of a comparison.  Ties that
the construction itself creates (neighbouring s2 both at the 1e-4 floor or both 1.0: sign(0) = 0 in SmoothLoss) are kept.

Saturation: the float64 reference must show 5 % .. 60 % of the elements on every saturated side of every clamp (asserted).

Every output buffer is filled with NaN and is one row longer than the contract: after the call the contracted elements are
finite and the extra row is untouched.  Every check prints `FIG <name> <backend> tol <t> err <e>`.

The bound the rule produced and the worst error seen on the emulator and on the MI355X (over the cases of each test) are in the
comment above each test."""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import zt_oracle as orc

NAN = float("nan")
U24 = 2.0 ** -24
F32, F64 = torch.float32, torch.float64


def rnd(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------ helpers
class Out:
    """NaN-filled output of the given shape followed by one more row of NaN (a row = the last dimension)"""

    def __init__(self, dev, *shape, dtype=F32, off_elems=0):
        self.n = int(math.prod(shape))
        self.raw = torch.full((off_elems + self.n + shape[-1],), NAN, dtype=dtype, device=dev)
        self.t = self.raw[off_elems: off_elems + self.n].view(*shape)
        self.tail = self.raw[off_elems + self.n:]
        self.head = self.raw[:off_elems]

    def check(self):
        assert bool(torch.isfinite(self.t).all()), "contracted elements not all written"
        assert bool(torch.isnan(self.tail).all()) and bool(torch.isnan(self.head).all()), "wrote outside the contract"
        return self.t


def rule_tol(ref64, ref32, extra=0.0):
    r64, r32 = ref64.detach().double().cpu(), ref32.detach().double().cpu()
    return max(8.0 * float((r32 - r64).abs().max()), 4.0 * U24 * float(r64.abs().max())) + extra


def check(name, backend, got, ref64, ref32, extra=0.0):
    """one tensor = one quantity"""
    got = got.detach().double().cpu().reshape(-1)
    r64 = ref64.detach().double().cpu().reshape(-1)
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    tol = rule_tol(ref64, ref32, extra)
    err = float((got - r64).abs().max())
    print("FIG %s %s tol %.3e err %.3e scale %.3e" % (name, backend, tol, err, float(r64.abs().max())))
    assert err <= tol, (name, err, tol)


def check_each(name, backend, got, ref64, ref32, extras=None):
    """a vector of scalars (loss terms, sums): every element is a quantity of its own"""
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu().reshape(-1) for t in (got, ref64, ref32))
    for i in range(r64.numel()):
        check("%s[%d]" % (name, i), backend, got[i], r64[i], r32[i], 0.0 if extras is None else extras[i])


def near(v, bound, rel=1e-4):
    return (v - bound).abs() <= rel * abs(bound)


def guard(inp, pre, bounds):
    """`pre(inp)` -> list of float64 pre-clamp tensors, each the shape of `inp` and monotone in it; moves (x 0.99) the elements of
    `inp` whose pre-clamp value lies within 1e-4 relative of a bound, then asserts that none is left"""
    for _ in range(8):
        bad = torch.zeros_like(inp, dtype=torch.bool)
        for v in pre(inp):
            for b in bounds:
                bad |= near(v, b)
        if not bool(bad.any()):
            break
        inp[bad] *= 0.99
    survivors = sum(int(near(v, b).sum()) for v in pre(inp) for b in bounds)
    assert survivors == 0, survivors
    return inp


def share(name, mask):
    """asserts the saturation condition on the float64 reference"""
    s = float(mask.double().mean())
    print("SHARE %s %.3f" % (name, s))
    assert 0.05 <= s <= 0.60, (name, s)


def pd(x):
    return orc.pair_downsample(x)


def nhwc(t):
    """[1,C,H,W] -> [H*W, C]"""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------ the loss, restated
def ef_ratio(L2, is_WB):
    """loss.py:26-37 in the dtype of L2 -> (pre-clamp ef, clamped ef, ratio), each [1,3,1,1]"""
    eps = 1e-9
    if is_WB:
        ef0 = (0.3 / (torch.mean(L2, dim=(2, 3)) + eps)).unsqueeze(2).unsqueeze(3)
    else:
        lum = L2[:, 2] * 0.299 + L2[:, 1] * 0.587 + L2[:, 0] * 0.144
        ef0 = (0.5 / (torch.mean(lum, dim=(1, 2)) + eps)).view(-1, 1, 1, 1).repeat(1, 3, 1, 1)
    ef = torch.clamp(ef0, 1, 25)
    return ef0, ef, torch.pow(0.7, -ef) / ef


def terms_s2(L2, s2, Y, is_WB):
    """terms 0-3 (loss.py:46-49); L2 detached (a constant here), s2 the leaf, Y the given luminance/chroma planes"""
    eps = 1e-9
    _, ef, ratio = ef_ratio(L2, is_WB)
    nl = torch.clamp(L2 / s2, eps, 0.8)
    ceb = torch.clamp(torch.pow(L2 * ef, ef) * ratio, eps, 1)
    cal = torch.clamp(L2 * ef, eps, 1)
    sm = 0.0
    for dy, dx in orc.SMOOTH_OFFSETS:
        ya, yb = orc._shift_pair(Y, dy, dx)
        oa, ob = orc._shift_pair(s2, dy, dx)
        w = torch.exp(((ya - yb) ** 2).sum(dim=1, keepdim=True) * (-1.0 / 200.0))
        sm = sm + 2.0 * (w * (oa - ob).abs().sum(dim=1, keepdim=True)).mean()
    return [F.mse_loss(s2, ceb) * 700, F.mse_loss(nl, cal) * 1000, sm * 5, orc.tv_loss(s2) * 1600]


HALF_IN = ["Lq11", "Lq12", "Lp1", "Lp2", "den1", "den2", "H3p", "H4p", "H11", "s21", "H12", "s22", "H3d1", "H3d2", "mask", "LM1", "LM2"]
HALF_LEAVES = ["Lp1", "Lp2", "den1", "den2", "H3p", "H4p", "H3d1", "H3d2", "LM1", "LM2"]
HALF_OUT = ["dLp1", "dLp2", "dden1", "dden2", "dH3p", "dH4p", "dH3d1", "dH3d2", "u1", "u2"]


def terms_half(d):
    """terms 4-11, 14, 15 (loss.py:51-62, 68-73); H11/s21/H12/s22 detached; LM1/LM2 leaves of their own; wd2 uses H3d1 (sic)"""
    mse, m = F.mse_loss, d["mask"]
    wd1 = (1 - m) * d["LM1"] + d["H3d1"] * m
    wd2 = (1 - m) * d["LM2"] + d["H3d1"] * m
    return [mse(d["Lq11"], d["Lp2"]) * 1000, mse(d["Lq12"], d["Lp1"]) * 1000, mse(d["Lp1"], d["den1"]) * 1000,
            mse(d["Lp2"], d["den2"]) * 1000,
            mse(d["H3p"], torch.cat([d["H12"], d["s22"]], 1)) * 1000, mse(d["H4p"], torch.cat([d["H11"], d["s21"]], 1)) * 1000,
            mse(d["H3p"][:, 0:3], d["H3d1"]) * 1000, mse(d["H4p"][:, 0:3], d["H3d2"]) * 1000,
            mse(d["H3d1"], wd1) * 10000, mse(d["H3d2"], wd2) * 10000]


def terms_full(H2b, H3b, s2, s3, VH2, VN):
    """terms 12, 13, 16 (loss.py:64, 66, 75-77)"""
    return [F.mse_loss(H2b, H3b) * 10000, F.mse_loss(s2, s3) * 1000, F.mse_loss(VH2, VN) * 1000]


def with_grads(fn, consts, leaves, dt):
    """-> (terms [k] in dt, {leaf: gradient of the sum of the terms})"""
    c = {k: v.to(dt) for k, v in consts.items()}
    lv = {k: v.to(dt).clone().requires_grad_(True) for k, v in leaves.items()}
    terms = fn(c, lv)
    torch.stack(terms).sum().backward()
    return torch.stack([t.detach() for t in terms]), {k: v.grad for k, v in lv.items()}


# ----------------------------------------------------------------------------- 1: plane sums -> enhancement scalars
def _scalars_ref(x, HW, is_WB, dt):
    """scal[0..5] by the definition, from the planes x [3, HW] in dtype dt"""
    _, ef, ratio = ef_ratio(x.to(dt).view(1, 3, 1, HW), is_WB)
    return torch.cat([ef.reshape(-1), ratio.reshape(-1)])


def _planes(seed, C, HW, scales):
    x = rnd(seed, C, HW)
    for c in range(C):
        x[c] *= scales[c % len(scales)]
    return x


def _guard_ef(x, is_WB):
    """channel means (or luminance mean) against the means that give ef = 1 and ef = 25"""
    for _ in range(8):
        ef0 = ef_ratio(x.double().view(1, 3, 1, -1), is_WB)[0].reshape(-1)
        bad = near(ef0, 1.0) | near(ef0, 25.0)
        if not bool(bad.any()):
            break
        if is_WB:
            x[bad] *= 0.99
        else:
            x *= 0.99
    ef0 = ef_ratio(x.double().view(1, 3, 1, -1), is_WB)[0].reshape(-1)
    assert not bool((near(ef0, 1.0) | near(ef0, 25.0)).any())
    return x, ef0


def _run_plane_sums(ops, dev, x, C, HW, nblk, off_bytes=0):
    raw = torch.empty(C * HW + 4, device=dev)
    assert raw.data_ptr() % 16 == 0
    xd = raw[off_bytes // 4: off_bytes // 4 + C * HW]
    xd.copy_(x.reshape(-1))
    part = Out(dev, nblk, C)
    ops.lib.call("zt_plane_sums_f32", xd, C, HW, nblk, part.t, ops._s(xd))
    return part.check()


# scalar levels of the non-WB sets: ef clamped at 25, un-clamped, clamped at 1; the WB set has one channel of each kind
LEVELS = {"lo": (0.02,), "mid": (0.5,), "hi": (1.9,), "wb": (0.01, 0.5, 1.9)}
SUM_CASES = [(4, 1, 0), (4096, 3, 0), (16388, 1, 0), (20000, 7, 0), (1000, 256, 0),     # vector path
             (1001, 2, 0), (4096, 3, 4)]                                                 # scalar path: HW % 4, base + 4 bytes


# rule: sums 2.4e-7 .. 1.3e-6 relative, scal 2.4e-7 .. 3.1e-6 relative.  Worst error, emulator = MI355X (same values): sums 8.4e-8
# relative (0.23 of the bound), scal 3.9e-7 relative (0.50 of the bound)
@pytest.mark.parametrize("level,is_WB", [("lo", 0), ("mid", 0), ("hi", 0), ("wb", 1)])
@pytest.mark.parametrize("HW,nblk,off", SUM_CASES)
def test_plane_sums_scalars(backend, HW, nblk, off, level, is_WB):
    ops, dev, name = backend
    x = _planes(200 + HW + nblk, 3, HW, LEVELS[level])
    x, ef0 = _guard_ef(x, is_WB)
    if level == "wb":
        assert ef0[0] > 25 and 1 < ef0[1] < 25 and ef0[2] < 1, ef0
    else:
        assert {"lo": ef0[0] > 25, "mid": 1 < ef0[0] < 25, "hi": ef0[0] < 1}[level], ef0
    part = _run_plane_sums(ops, dev, x, 3, HW, nblk, off)
    check_each("plane_sums", name, part.double().sum(0), x.double().sum(1), x.sum(1))
    scal = Out(dev, 6)
    ops.lib.call("zt_loss_scalars_f32", part, nblk, HW, is_WB, scal.raw, ops._s(part))
    assert bool(torch.isfinite(scal.raw[:6]).all()) and bool(torch.isnan(scal.raw[8:]).all())      # scal[6], scal[7] are spare
    check_each("loss_scalars", name, scal.raw[:6], _scalars_ref(x, HW, is_WB, F64), _scalars_ref(x, HW, is_WB, F32))


# rule: 2.4e-7 .. 8.1e-7 relative.  Worst error, emulator = MI355X: 4.4e-8 relative (0.18 of the bound)
@pytest.mark.parametrize("C,HW,nblk", [(1, 16388, 1), (4, 16388, 1), (1, 20000, 7), (4, 20000, 7), (4, 1000, 256), (5, 4096, 3),
                                       (5, 1001, 2)])
def test_plane_sums_channels(backend, C, HW, nblk):
    """C = 1 and 4 on the vector path, C = 5 on the scalar path (C = 3 above)"""
    ops, dev, name = backend
    x = _planes(230 + C + HW, C, HW, (1.0, 0.1, 3.0))
    part = _run_plane_sums(ops, dev, x, C, HW, nblk)
    check_each("plane_sums_C", name, part.double().sum(0), x.double().sum(1), x.sum(1))


# --------------------------------------------------------------------------------------------- the loss's input sets
_SETS = {}


def loss_set(H, W, kind):
    """All tensors LossFunction.forward reads, fp32 on the CPU, saturating the clamps of terms 0-3.  kind: "wb25" (channel 0 of
    L2 scaled so that its WB enhancement factor clamps at 25), "mid" (un-clamped factor), "one" (mean drives the factor to 1)."""
    key = (H, W, kind)
    if key in _SETS:
        return _SETS[key]
    sd = 1000 + 7 * H + W
    h, w = H // 2, W // 2
    L2 = rnd(sd, 1, 3, H, W) ** 4
    s2 = rnd(sd + 2, 1, 3, H, W)
    if kind == "one":                                                # luminance mean above 0.5; s2 raised to keep L2 / s2 mixed
        L2, s2 = 0.35 + 0.85 * rnd(sd, 1, 3, H, W) ** 2, 0.3 + 0.7 * s2
    L2[rnd(sd + 1, 1, 3, H, W) < 0.08] = 0.0                          # lower side of clamp(.., 1e-9, ..)
    if kind == "wb25":
        L2[:, 0] *= 0.02
    s2[rnd(sd + 4, 1, 3, H, W) < 0.08] = 1e-4                        # the Enhancer's clamp floor
    s2[rnd(sd + 3, 1, 3, H, W) > 0.9] = 1.0                          # plateau
    for _ in range(3):                                               # the two guards move each other's quantity a little
        for is_WB in {"wb25": (1,), "mid": (0, 1), "one": (0,)}[kind]:
            _guard_ef(L2.view(3, -1), is_WB)                         # in place
        L2 = guard(L2, lambda t: [t.double() / s2.double()], (1e-9, 0.8))
    d = dict(L2=L2, s2=s2, Y=orc.ycc_flat(L2))
    for i, k in enumerate(["inp", "H2", "H3", "s3", "H2b", "H3b"]):
        d[k] = rnd(sd + 10 + i, 1, 3, H, W)
    for i, k in enumerate(["Lp1", "Lp2", "s21", "s22", "H11", "H12"]):
        d[k] = rnd(sd + 20 + i, 1, 3, h, w)
    d["H3p"], d["H4p"] = rnd(sd + 30, 1, 6, h, w), rnd(sd + 31, 1, 6, h, w)
    d["m_h"] = (rnd(sd + 32, 1, 1, h, w) > 0.5).float()
    _SETS[key] = d
    return d


def s2_saturation(d, is_WB, kind):
    L2, s2 = d["L2"].double(), d["s2"].double()
    ef0, ef, ratio = ef_ratio(L2, is_WB)
    for c in range(3):
        assert not bool(near(ef0[0, c, 0, 0], 1.0)) and not bool(near(ef0[0, c, 0, 0], 25.0))
    if kind == "wb25":
        assert float(ef0[0, 0, 0, 0]) > 25 and 1 < float(ef0[0, 1, 0, 0]) < 25
    elif kind == "one":
        assert float(ef0.max()) < 1
    else:
        assert 1 < float(ef0.min()) and float(ef0.max()) < 25
    q = L2 / s2
    assert int((near(q, 1e-9) | near(q, 0.8)).sum()) == 0
    if L2.shape[2] * L2.shape[3] < 64:                               # 27 elements cannot show a share
        return
    tag = "s2_%s_%dx%d_wb%d_" % (kind, L2.shape[2], L2.shape[3], is_WB)
    share(tag + "L2/s2>0.8", q > 0.8)
    share(tag + "L2/s2<1e-9", q < 1e-9)
    share(tag + "L2*ef>1", L2 * ef > 1)
    share(tag + "L2*ef<1e-9", L2 * ef < 1e-9)
    share(tag + "ceb>1", torch.pow(L2 * ef, ef) * ratio > 1)
    share(tag + "ceb<1e-9", torch.pow(L2 * ef, ef) * ratio < 1e-9)
    share(tag + "s2=floor", d["s2"] == 1e-4)
    share(tag + "s2=1", d["s2"] == 1.0)


_S2REF = {}


def s2_reference(H, W, kind, is_WB):
    key = (H, W, kind, is_WB)
    if key not in _S2REF:
        d = loss_set(H, W, kind)
        s2_saturation(d, is_WB, kind)
        fn = lambda c, lv: terms_s2(c["L2"], lv["s2"], c["Y"], is_WB)
        consts, leaves = dict(L2=d["L2"], Y=d["Y"]), dict(s2=d["s2"])
        _S2REF[key] = with_grads(fn, consts, leaves, F64) + with_grads(fn, consts, leaves, F32)
    return _S2REF[key]


def _scal_from_kernels(ops, dev, L2d, HW, is_WB):
    part = torch.full((1, 3), NAN, device=dev)
    ops.lib.call("zt_plane_sums_f32", L2d, 3, HW, 1, part, ops._s(L2d))
    scal = torch.full((8,), NAN, device=dev)
    ops.lib.call("zt_loss_scalars_f32", part, 1, HW, is_WB, scal, ops._s(L2d))
    return scal


S2_SHAPES = [(3, 3), (16, 64), (17, 65), (22, 130)]
S2_SETS = [("wb25", 1), ("mid", 0), ("mid", 1), ("one", 0)]


# rule: terms 2.4e-7 .. 1.5e-6 relative (2.0e-6 for smooth with fast_exp), ds2 3.6e-7 .. 3.1e-6 of its maximum (the fast_exp share is
# below 1e-9 of it).  Worst error, both fast_exp values: terms 1.7e-7 relative (0.54 of the bound) on the emulator and on the MI355X;
# ds2 3.3e-7 of its maximum on both, 0.79 of the bound (3x3: 27 elements, where float32 torch itself lands within 4.4e-8 of float64,
# so that the bound is 3.6e-7 of the largest gradient, 1.5 times the floor)
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("kind,is_WB", S2_SETS)
@pytest.mark.parametrize("H,W", S2_SHAPES)
def test_loss_s2(backend, H, W, kind, is_WB, fast):
    ops, dev, name = backend
    d = loss_set(H, W, kind)
    t64, g64, t32, g32 = s2_reference(H, W, kind, is_WB)
    L2, s2, Y = d["L2"].to(dev), d["s2"].to(dev), d["Y"].to(dev)
    scal = _scal_from_kernels(ops, dev, L2, H * W, is_WB)
    nb = ((W + 63) // 64) * ((H + 3) // 4)
    ds2, part = Out(dev, 1, 3, H, W), Out(dev, nb, 4)
    ops.lib.call("zt_loss_s2_f32", L2, s2, Y, scal, H, W, ds2.t, part.t, fast, ops._s(L2))
    terms = part.check().double().sum(0)
    coef = sum(2 * 10.0 / ((H - dy) * (W - abs(dx))) for dy, dx in orc.SMOOTH_OFFSETS)
    ex = 2.0 ** -21 if fast else 0.0
    check_each("loss_s2_terms_fast%d" % fast, name, terms, t64, t32, [0.0, 0.0, ex * float(t64[2].abs()), 0.0])
    check("loss_s2_ds2_fast%d" % fast, name, ds2.check(), g64["s2"], g32["s2"], ex * coef)


# --------------------------------------------------------------------------------------------------- 3: half-res terms
def half_inputs(hw, mask_kind):
    d = {k: rnd(300 + i + hw, 1, 6 if k in ("H3p", "H4p") else 3, 1, hw) for i, k in enumerate(HALF_IN) if k != "mask"}
    m = (rnd(340 + hw, 1, 1, 1, hw) > 0.5).float()
    d["mask"] = {"mixed": m, "zeros": torch.zeros_like(m), "ones": torch.ones_like(m)}[mask_kind]
    return d


def half_reference(d, dt):
    consts = {k: v for k, v in d.items() if k not in HALF_LEAVES}
    leaves = {k: d[k] for k in HALF_LEAVES}
    t, g = with_grads(lambda c, lv: terms_half({**c, **lv}), consts, leaves, dt)
    g["u1"], g["u2"] = -g.pop("LM1"), -g.pop("LM2")
    return t, {("d" + k if not k.startswith("u") else k): v for k, v in g.items()}


def run_loss_half(ops, dev, d, hw):
    ins = [d[k].to(dev).contiguous() for k in HALF_IN]
    outs = {k: Out(dev, 1, 6 if k in ("dH3p", "dH4p") else 3, 1, hw) for k in HALF_OUT}
    nb = (hw + 255) // 256
    part = Out(dev, nb, 10)
    ops.lib.call("zt_loss_half_f32", *ins, *[outs[k].t for k in HALF_OUT], hw, part.t, ops._s(ins[0]))
    return part.check().double().sum(0), {k: v.check() for k, v in outs.items()}


# rule: terms 2.4e-7 .. 1.3e-6 relative (0 where the term is exactly 0: inter_a with an all-ones mask), gradients 2.4e-7 .. 9.7e-7 of
# their maximum.  Worst error, emulator = MI355X: terms 1.2e-7 relative (0.47 of the bound), gradients 1.1e-7 (0.34 of the bound)
@pytest.mark.parametrize("mask_kind", ["mixed", "zeros", "ones"])
@pytest.mark.parametrize("hw", [1, 255, 256, 257, 1000])
def test_loss_half(backend, hw, mask_kind):
    ops, dev, name = backend
    d = half_inputs(hw, mask_kind)
    t64, g64 = half_reference(d, F64)
    t32, g32 = half_reference(d, F32)
    terms, grads = run_loss_half(ops, dev, d, hw)
    check_each("loss_half_terms", name, terms, t64, t32)
    for k in HALF_OUT:
        check("loss_half_" + k, name, grads[k], g64[k], g32[k])


# --------------------------------------------------------------------------------------------------- 4: full-res terms
FULL_IN = ["H2b", "H3b", "s2", "s3", "VH2", "VN"]


def full_reference(d, dt):
    fn = lambda c, lv: terms_full(c["H2b"], lv["H3b"], c["s2"], lv["s3"], lv["VH2"], c["VN"])
    return with_grads(fn, {k: d[k] for k in ("H2b", "s2", "VN")}, {k: d[k] for k in ("H3b", "s3", "VH2")}, dt)


# rule: terms 2.4e-7 .. 6.9e-7 relative, gradients 2.4e-7 .. 5.8e-7 of their maximum.  Worst error, emulator = MI355X: terms 8.4e-8
# relative (0.35 of the bound), gradients 8.0e-8 (0.16 of the bound)
@pytest.mark.parametrize("n", [1, 256, 257, 999])
def test_loss_full(backend, n):
    ops, dev, name = backend
    d = {k: rnd(400 + i + n, n) for i, k in enumerate(FULL_IN)}
    (t64, g64), (t32, g32) = full_reference(d, F64), full_reference(d, F32)
    outs = {k: Out(dev, n) for k in ("dH3b", "ds3", "gV")}
    part = Out(dev, (n + 255) // 256, 3)
    ops.lib.call("zt_loss_full_f32", *[d[k].to(dev) for k in FULL_IN], outs["dH3b"].t, outs["ds3"].t, outs["gV"].t, n, part.t,
                 ops._s(part.t))
    check_each("loss_full_terms", name, part.check().double().sum(0), t64, t32)
    for k, leaf in (("dH3b", "H3b"), ("ds3", "s3"), ("gV", "VH2")):
        check("loss_full_" + k, name, outs[k].check(), g64[leaf], g32[leaf])


# ------------------------------------------------------------------------------------------------------ 5: composition
TERM_NAMES = ["enh_s2", "enh_norm", "smooth", "tv", "res1_a", "res1_b", "res1_c", "res1_d", "res2_a", "res2_b", "res2_c", "res2_d",
              "color", "ill", "inter_a", "inter_b", "var"]


def _oracle_terms(d, is_WB, dt):
    c = {k: v.to(dt) for k, v in d.items()}
    outs = (c["Lp1"], c["Lp2"], c["L2"], c["s2"], c["s21"], c["s22"], c["H2"], c["H11"], c["H12"], c["H3p"][:, :3], c["H3p"][:, 3:],
            c["H4p"][:, :3], c["H4p"][:, 3:], c["H3"], c["s3"], c["H3p"], c["H4p"], None, c["m_h"], c["H2b"], c["H3b"])
    total, t = orc.loss_terms(c["inp"], outs, bool(is_WB))
    return torch.stack([t[k] for k in TERM_NAMES] + [total])


def _restated_terms(d, is_WB):
    """the 17 terms through terms_s2 / terms_half / terms_full in float64, the way the kernels split them"""
    c = {k: v.double() for k, v in d.items()}
    Lq11, Lq12 = pd(c["inp"] + 1e-9)
    den1, den2 = pd(c["L2"])
    H3d1, H3d2 = pd(c["H3"])
    half = dict(Lq11=Lq11, Lq12=Lq12, Lp1=c["Lp1"], Lp2=c["Lp2"], den1=den1, den2=den2, H3p=c["H3p"], H4p=c["H4p"], H11=c["H11"],
                s21=c["s21"], H12=c["H12"], s22=c["s22"], H3d1=H3d1, H3d2=H3d2, mask=c["m_h"], LM1=orc.local_mean_reflect(H3d1),
                LM2=orc.local_mean_reflect(H3d2))
    a, b = terms_s2(c["L2"], c["s2"], c["Y"], is_WB), terms_half(half)
    f = terms_full(c["H2b"], c["H3b"], c["s2"], c["s3"], orc.local_variance_zero(c["H2"]), orc.local_variance_zero(c["H3"] - c["H2"]))
    return torch.stack(a + b[:8] + f[:2] + b[8:] + f[2:])


# rule: 2.4e-7 .. 1.3e-6 relative per term.  Worst error 1.3e-7 relative on both; 0.36 of the bound on the emulator, 0.38 on the MI355X
@pytest.mark.parametrize("kind,is_WB", [("wb25", 1), ("mid", 0), ("one", 0)])
@pytest.mark.parametrize("H,W", [(22, 70), (16, 64)])
def test_loss_composition(backend, H, W, kind, is_WB):
    ops, dev, name = backend
    d = loss_set(H, W, kind)
    s2_saturation(d, is_WB, kind)
    r64, r32 = _oracle_terms(d, is_WB, F64), _oracle_terms(d, is_WB, F32)
    # the restatement the gradient tests differentiate is the oracle's loss: 1e-12 relative (smooth: the oracle's Y is fp32)
    mine = _restated_terms(d, is_WB)
    for i, k in enumerate(TERM_NAMES):
        assert abs(float(mine[i] - r64[i])) <= (1e-6 if k == "smooth" else 1e-12) * abs(float(r64[i])), (k, mine[i], r64[i])
    engine = importlib.import_module("zero-tig_amd.engine")
    t = {k: v.to(dev) for k, v in d.items()}
    loss, terms = engine.loss_value(ops, bool(is_WB), t["inp"], t["Lp1"], t["Lp2"], t["L2"], t["s2"], t["s21"], t["s22"], t["H2"],
                                    t["H11"], t["H12"], t["H3"], t["s3"], t["H3p"], t["H4p"], t["m_h"], t["H2b"], t["H3b"])
    assert terms.shape == (17,) and bool(torch.isfinite(terms).all())
    check_each("composition", name, torch.cat([terms.reshape(-1), loss.reshape(-1)]), r64, r32)


# ------------------------------------------------------------------------------------------------ 6 / 7: glue inputs
GLUE_SHAPES = [(2, 2), (8, 128), (10, 130), (12, 258)]
_GLUE = {}


def glue_set(H, W):
    """inputs of the element-wise stages with every clamp of model.py:145-199 saturated on both sides"""
    key = (H, W)
    if key in _GLUE:
        return _GLUE[key]
    sd = 5000 + 11 * H + W
    h, w = H // 2, W // 2
    big = H * W >= 64                                                # a 2 x 2 image cannot show a share
    d = {}
    d["inp"] = rnd(sd, 1, 3, H, W)
    x = rnd(sd + 1, 1, 3, H, W) * 0.8
    x[rnd(sd + 2, 1, 3, H, W) < 0.1] = 1e-6                          # x / s2 below 1e-4
    s2 = rnd(sd + 3, 1, 3, H, W)
    s2[s2 < 0.08] = 1e-4
    s2[rnd(sd + 4, 1, 3, H, W) > 0.9] = 1.0
    d["s2"] = s2
    s21, s22 = pd(s2)                                                # fp32, the kernel's own expression (bit-equal, case 6)
    d["s21"], d["s22"] = s21, s22
    d["x"] = guard(x, lambda t: [t.double() / s2.double()], (1e-4, 1.0))
    for k, sk, o in (("L11", s21, 5), ("L12", s22, 7)):
        L = rnd(sd + o, 1, 3, h, w) * 0.8
        L[rnd(sd + o + 1, 1, 3, h, w) < 0.1] = 1e-6
        d[k] = guard(L, lambda t, sk=sk: [t.double() / sk.double()], (1e-4, 1.0))
    n = rnd(sd + 9, 1, 3, H, W) * 1.6 - 0.5                          # x - n leaves [1e-4, 1] on both sides
    xn = rnd(sd + 10, 1, 3, H, W)
    d["n"] = -guard(-n, lambda t: [xn.double() + t.double()], (1e-4, 1.0))
    d["xn"] = xn
    L2 = rnd(sd + 11, 1, 3, H, W) * 1.2 - 0.1                        # H1 = clamp(L2 / s2, 0, 1): below 0 and above 1
    d["L2"] = guard(L2, lambda t: [t.double() / s2.double()], (0.0, 1.0))
    d["n11"], d["n12"] = rnd(sd + 12, 1, 3, h, w) - 0.5, rnd(sd + 13, 1, 3, h, w) - 0.5
    A, B = rnd(sd + 14, 1, 3, H, W), rnd(sd + 15, 1, 3, H, W)
    r = rnd(sd + 16, 1, 6, H, W) * 1.6 - 0.5                         # A - r leaves [1e-4, 1] on both sides
    AB = torch.cat([A, B], 1)
    d["r"] = -guard(-r, lambda t: [AB.double() + t.double()], (1e-4, 1.0))
    d["A"], d["B"] = A, B
    for i, k in enumerate(["gA", "gB", "dH2x", "ds2d"]):
        d[k] = rnd(sd + 20 + i, 1, 3, H, W) - 0.5
    d["dIn5"] = rnd(sd + 25, 1, 12, H, W) - 0.5
    d["dIn3"], d["dIn4"] = rnd(sd + 26, 1, 12, h, w) - 0.5, rnd(sd + 27, 1, 12, h, w) - 0.5
    for i, k in enumerate(["dLp1", "dLp2", "dden1", "dden2"]):
        d[k] = rnd(sd + 30 + i, 1, 3, h, w) - 0.5
    if big:
        tag = "glue_%dx%d_" % (H, W)
        for nm, v, lo in (("x/s2", d["x"].double() / s2.double(), 1e-4), ("L11/s21", d["L11"].double() / s21.double(), 1e-4),
                          ("L12/s22", d["L12"].double() / s22.double(), 1e-4), ("x-n", xn.double() - d["n"].double(), 1e-4),
                          ("A-r", AB.double() - d["r"].double(), 1e-4), ("L2/s2", d["L2"].double() / s2.double(), 0.0)):
            share(tag + nm + "<lo", v < lo)
            share(tag + nm + ">1", v > 1.0)
        share(tag + "s2=floor", s2 == 1e-4)
        share(tag + "s2=1", s2 == 1.0)
    _GLUE[key] = d
    return d


def same(name, backend, got, ref_fn, *ins):
    """bit-equal to the expression in float32 torch, and within the rule of the same expression in float64"""
    r32 = ref_fn(*ins)
    r64 = ref_fn(*[t.double() for t in ins])
    r32, r64 = (r if isinstance(r, (tuple, list)) else (r,) for r in (r32, r64))
    got = got if isinstance(got, (tuple, list)) else (got,)
    assert len(got) == len(r32)
    for i, (g, a, b) in enumerate(zip(got, r32, r64)):
        assert a.dtype == F32 and b.dtype == F64
        check("%s[%d]" % (name, i), backend, g, b, a)
        assert torch.equal(g.cpu().reshape(a.shape), a), (name, i)


def _ref_prep(inp):
    x = inp + 1e-4
    return (x,) + tuple(pd(x)) + tuple(pd(inp + 1e-9))


def _ref_d1_tail(x, n, L11, n11, L12, n12):
    L2 = torch.clamp(x - n, 1e-4, 1)
    return (L2, L11 - n11, L12 - n12) + tuple(pd(L2))


def _ref_post_enh(x, s2, L2, L11, L12):
    s21, s22 = pd(s2)
    return (s21, s22, torch.clamp(x / s2, 1e-4, 1), torch.clamp(L11 / s21, 1e-4, 1), torch.clamp(L12 / s22, 1e-4, 1),
            torch.clamp(L2 / s2, 0, 1))


def _ref_sub6(A, B, r):
    return torch.clamp(A - r[:, :3], 1e-4, 1), torch.clamp(B - r[:, 3:], 1e-4, 1)


# bit-equal to float32 torch on the emulator and on the MI355X (the rule gives 2.4e-7 .. 6.4e-7 relative; error 1/8 of it by construction)
@pytest.mark.parametrize("H,W", GLUE_SHAPES)
def test_glue_forward(backend, H, W):
    ops, dev, name = backend
    d = glue_set(H, W)
    h, w = H // 2, W // 2
    t = {k: v.to(dev) for k, v in d.items()}
    s = ops._s(t["x"])
    full, half = (lambda: Out(dev, 1, 3, H, W)), (lambda: Out(dev, 1, 3, h, w))

    o = [full(), half(), half(), half(), half()]
    ops.lib.call("zt_prep_input_f32", t["inp"], *[b.t for b in o], H, W, s)
    same("prep_input", name, [b.check() for b in o], _ref_prep, d["inp"])

    o = [full(), half(), half(), half(), half()]
    ops.lib.call("zt_d1_tail_f32", t["xn"], t["n"], t["L11"], t["n11"], t["L12"], t["n12"], *[b.t for b in o], H, W, s)
    same("d1_tail", name, [b.check() for b in o], _ref_d1_tail, d["xn"], d["n"], d["L11"], d["n11"], d["L12"], d["n12"])

    o = [half(), half(), full(), half(), half(), full()]
    ops.lib.call("zt_post_enh_f32", t["x"], t["s2"], t["L2"], t["L11"], t["L12"], *[b.t for b in o], H, W, s)
    same("post_enh", name, [b.check() for b in o], _ref_post_enh, d["x"], d["s2"], d["L2"], d["L11"], d["L12"])

    o = [full(), full()]
    ops.lib.call("zt_clamp_sub6_f32", t["A"], t["B"], t["r"], o[0].t, o[1].t, H * W, s)
    same("clamp_sub6", name, [b.check() for b in o], _ref_sub6, d["A"], d["B"], d["r"])


# bit-equal to float32 torch on the emulator and on the MI355X (rule: 2.4e-7 .. 6.2e-7 relative)
@pytest.mark.parametrize("n", [1, 257])
def test_glue_flat(backend, n):
    ops, dev, name = backend
    a, b, c = rnd(600 + n, n) * 2.2 - 0.4, rnd(601 + n, n) * 0.9 + 0.3, rnd(602 + n, n) - 0.5
    b[::10] = 1e-4
    ta, tb, tc = a.to(dev), b.to(dev), c.to(dev)
    s = ops._s(ta)

    def run(fn_name, *args):
        o = Out(dev, n)
        ops.lib.call(fn_name, *[o.t if x is Ellipsis else x for x in args], s)
        return o.check()

    same("ew0", name, run("zt_ew_f32", ta, None, ..., 0, 1e-4, 0.0, n), lambda a: a + 1e-4, a)
    same("ew1", name, run("zt_ew_f32", ta, tb, ..., 1, 1e-4, 1.0, n), lambda a, b: torch.clamp(a - b, 1e-4, 1.0), a, b)
    same("ew2", name, run("zt_ew_f32", ta, tb, ..., 2, 1e-4, 1.0, n), lambda a, b: torch.clamp(a / b, 1e-4, 1.0), a, b)
    if n > 1:                                                        # one element cannot show a share
        q, df = a.double() / b.double(), a.double() - b.double()
        assert not bool((near(q, 1e-4) | near(q, 1.0) | near(df, 1e-4) | near(df, 1.0)).any())
        share("ew_a/b<1e-4", q < 1e-4), share("ew_a/b>1", q > 1), share("ew_a-b<1e-4", df < 1e-4), share("ew_a-b>1", df > 1)
    al, be = 0.3, -1.7
    al32, be32 = float(torch.tensor(al, dtype=F32)), float(torch.tensor(be, dtype=F32))      # the values the kernel receives
    same("axpby", name, run("zt_axpby_f32", ta, tb, ..., al, be, n), lambda a, b: al32 * a + be32 * b, a, b)
    same("add3", name, run("zt_add3_f32", ta, tb, tc, ..., n), lambda a, b, c: a + b + c, a, b, c)
    same("add3_null", name, run("zt_add3_f32", ta, tb, None, ..., n), lambda a, b: a + b, a, b)
    # y <- fma(alpha, x, y): one rounding; the float64 expression rounded once is that value
    alpha = torch.tensor([al], dtype=F32)
    y = Out(dev, n)
    y.t.copy_(tc)
    ops.lib.call("zt_axpy_dev_f32", y.t, ta, alpha.to(dev), n, s)
    r64 = alpha.double() * a.double() + c.double()
    check("axpy_dev", name, y.check(), r64, r64.float())
    assert torch.equal(y.t.cpu(), r64.float())


# ------------------------------------------------------------------------------------------------- 7: glue backward
def _sub6_bwd_ref(d, dt):
    A, B, gA, gB = (d[k].to(dt) for k in ("A", "B", "gA", "gB"))
    r = d["r"].to(dt).clone().requires_grad_(True)
    oA, oB = _ref_sub6(A, B, r)
    ((oA * gA).sum() + (oB * gB).sum()).backward()
    return nhwc(r.grad)


# gradients are -g or 0: the rule gives its floor, 2.4e-7 of max|g|; error 0 on the emulator and on the MI355X
@pytest.mark.parametrize("H,W", GLUE_SHAPES)
def test_clamp_sub6_bwd(backend, H, W):
    ops, dev, name = backend
    d = glue_set(H, W)
    t = {k: d[k].to(dev) for k in ("A", "B", "r", "gA", "gB")}
    dr = Out(dev, H * W, 8)
    ops.lib.call("zt_clamp_sub6_bwd", t["A"], t["B"], t["r"], t["gA"], t["gB"], dr.t, 0, 8, H * W, ops._s(dr.t))
    got = dr.check()
    check("clamp_sub6_bwd", name, got[:, :6], _sub6_bwd_ref(d, F64), _sub6_bwd_ref(d, F32))
    assert torch.equal(got[:, 6:].cpu(), torch.zeros(H * W, 2))


def _d1_bwd_ref(d, dt):
    c = {k: d[k].to(dt) for k in ("xn", "L11", "L12", "dLp1", "dLp2", "dden1", "dden2")}
    lv = {k: d[k].to(dt).clone().requires_grad_(True) for k in ("n", "n11", "n12")}
    _, Lp1, Lp2, den1, den2 = _ref_d1_tail(c["xn"], lv["n"], c["L11"], lv["n11"], c["L12"], lv["n12"])
    ((Lp1 * c["dLp1"]).sum() + (Lp2 * c["dLp2"]).sum() + (den1 * c["dden1"]).sum() + (den2 * c["dden2"]).sum()).backward()
    return [nhwc(lv[k].grad) for k in ("n", "n11", "n12")]


# gradients are -g/2, -g or 0: the rule gives its floor, 2.4e-7 of max|g|; error 0 on the emulator and on the MI355X
@pytest.mark.parametrize("H,W", GLUE_SHAPES)
def test_d1_bwd_prep(backend, H, W):
    ops, dev, name = backend
    d = glue_set(H, W)
    h, w = H // 2, W // 2
    t = {k: d[k].to(dev) for k in ("xn", "n", "dLp1", "dLp2", "dden1", "dden2")}
    outs = [Out(dev, H * W, 4), Out(dev, h * w, 4), Out(dev, h * w, 4)]
    ops.lib.call("zt_d1_bwd_prep", t["xn"], t["n"], t["dLp1"], t["dLp2"], t["dden1"], t["dden2"], *[o.t for o in outs], 0, 4, H, W,
                 ops._s(t["n"]))
    r64, r32 = _d1_bwd_ref(d, F64), _d1_bwd_ref(d, F32)
    for k, o, a, b in zip(("dn", "dn11", "dn12"), outs, r64, r32):
        got = o.check()
        check("d1_bwd_prep_" + k, name, got[:, :3], a, b)
        assert torch.equal(got[:, 3].cpu(), torch.zeros(got.shape[0]))


def _post_enh_bwd_ref(d, dt):
    """-> (gradient w.r.t. s2 [1,3,H,W], dO [H*W,3]) of the forward model.py:169-177 written with the oracle's pair_downsample"""
    c = {k: d[k].to(dt) for k in ("x", "L11", "L12", "dIn5", "dH2x", "dIn3", "dIn4", "ds2d")}
    s2 = d["s2"].to(dt).clone().requires_grad_(True)
    s21, s22 = pd(s2)
    H2, H11, H12 = torch.clamp(c["x"] / s2, 1e-4, 1), torch.clamp(c["L11"] / s21, 1e-4, 1), torch.clamp(c["L12"] / s22, 1e-4, 1)
    tot = (c["ds2d"] * s2).sum() + (c["dIn5"][:, 6:9] * H2).sum() + (c["dIn5"][:, 9:12] * s2).sum() + (c["dH2x"] * H2).sum()
    tot = tot + (c["dIn3"][:, 6:9] * H11).sum() + (c["dIn3"][:, 9:12] * s21).sum()
    tot = tot + (c["dIn4"][:, 6:9] * H12).sum() + (c["dIn4"][:, 9:12] * s22).sum()
    tot.backward()
    g, s = s2.grad, s2.detach()
    return g, nhwc(g * s * (1 - s) * (s > 1e-4).to(dt))


# rule: ds2_total 4.5e-7 .. 1.0e-6 of its maximum, dO 5.3e-7 .. 1.0e-6.  Worst error, emulator = MI355X: ds2_total 1.3e-7 (0.125 of the
# bound: bit-equal to float32 autograd), dO 1.0e-7 (0.15 of the bound).  max|ds2_total| is 70 .. 80 here (x = 1e-6 over s2 = 1e-4 gives
# -x / s2^2 = -100), so the bound is 4e-5 .. 9e-5 absolute while an ordinary gradient is O(1): ordinary elements have that much slack
@pytest.mark.parametrize("H,W", GLUE_SHAPES)
def test_post_enh_bwd(backend, H, W):
    ops, dev, name = backend
    d = glue_set(H, W)
    t = {k: d[k].to(dev) for k in ("x", "s2", "L11", "L12", "s21", "s22", "dIn5", "dH2x", "dIn3", "dIn4", "ds2d")}
    args = [t[k] for k in ("x", "s2", "L11", "L12", "s21", "s22", "dIn5", "dH2x", "dIn3", "dIn4", "ds2d")]
    dO, tot = Out(dev, H * W, 4), Out(dev, 1, 3, H, W)
    ops.lib.call("zt_post_enh_bwd", *args, dO.t, 0, 4, tot.t, H, W, ops._s(dO.t))
    (g64, o64), (g32, o32) = _post_enh_bwd_ref(d, F64), _post_enh_bwd_ref(d, F32)
    got = dO.check()
    check("post_enh_bwd_ds2_total", name, tot.check(), g64, g32)
    check("post_enh_bwd_dO", name, got[:, :3], o64, o32)
    assert torch.equal(got[:, 3].cpu(), torch.zeros(H * W))
    floor = nhwc(d["s2"] <= 1e-4)
    assert torch.equal(got[:, :3].cpu()[floor], torch.zeros(int(floor.sum())))          # exactly zero at the Enhancer's floor
    dO2 = Out(dev, H * W, 4)
    ops.lib.call("zt_post_enh_bwd", *args, dO2.t, 0, 4, None, H, W, ops._s(dO.t))
    assert torch.equal(dO2.check(), got)


# out = g or 0: exact
@pytest.mark.parametrize("dtype", [F32, torch.bfloat16])
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("npix", [1, 257])
def test_relu_mask(backend, npix, pad, dtype):
    ops, dev, name = backend
    C, ld = 64, 64 + pad
    g = (rnd(700 + npix, npix, ld) - 0.5).to(dtype)
    a = (rnd(701 + npix, npix, ld) - 0.5).to(dtype)
    a[:, 0::7], a[:, 3::7] = 0.0, -0.0
    assert bool((a == 0).any()) and bool(torch.signbit(a[a == 0]).any()) and not bool(torch.signbit(a[a == 0]).all())
    out = Out(dev, npix, ld, dtype=dtype)
    ops.lib.call("zt_relu_mask_nhwc", g.to(dev), 1 if dtype == torch.bfloat16 else 0, ld, a.to(dev), ld, out.t, ld, npix, C,
                 ops._s(out.t))
    assert bool(torch.isnan(out.tail).all())
    got = out.t.cpu()
    assert bool(torch.isfinite(got[:, :C]).all()) and bool(torch.isnan(got[:, C:]).all())          # pad channels are not the kernel's
    a64 = a[:, :C].double().requires_grad_(True)
    (torch.relu(a64) * g[:, :C].double()).sum().backward()
    assert torch.equal(got[:, :C].double(), a64.grad)


# ------------------------------------------------------------------------------------------------------------ 8: pack
PACK_CASES = [(0, 4, (3,), 0), (0, 12, (3, 3, 3, 3), 0), (1, 8, (3,), 0), (1, 8, (3, 3), 0), (1, 16, (3, 3, 3, 3), 0),
              (1, 12, (3, 3, 3), 0), (1, 8, (3, 3), 8)]


# values are the sources rounded to the storage type: exact
@pytest.mark.parametrize("HW", [1, 255, 257])
@pytest.mark.parametrize("dt,ld,groups,off", PACK_CASES)
def test_pack_nhwc(backend, dt, ld, groups, off, HW):
    ops, dev, name = backend
    dtype = torch.bfloat16 if dt else F32
    srcs = [rnd(800 + 10 * i + HW, c, HW) - 0.5 for i, c in enumerate(groups)]
    dst = Out(dev, HW, ld, dtype=dtype, off_elems=off // 2 if dt else off // 4)
    assert dst.raw.data_ptr() % 16 == 0 and dst.t.data_ptr() % 16 == off
    a = []
    for j in range(4):
        a += [srcs[j].to(dev), groups[j]] if j < len(groups) else [None, 0]
    ops.lib.call("zt_pack_nhwc", dst.t, dt, ld, HW, *a, ops._s(dst.t))
    got = dst.check().cpu()
    ref = torch.cat(srcs, 0).t().contiguous()                        # [HW, sum c]
    nch = ref.shape[1]
    assert torch.equal(got[:, :nch], ref.to(dtype))
    assert torch.equal(got[:, nch:], torch.zeros(HW, ld - nch, dtype=dtype))


# ---------------------------------------------------------------------------------------------------- 9: clip + Adam
# The C ABI carries the betas as fp32, so the kernel runs Adam with beta1 = fp32(0.9), beta2 = fp32(0.999) = 0.99900001287...: those
# are its input values, and the references receive the same ones ("built from the same fp32 input values").  With beta2 = 0.999 in
# double torch's 1 - beta2 is 1.3e-5 away from the kernel's 1.f - 0.999f, which says nothing about the kernel's arithmetic.
LR, ADAM_EPS = 1e-4, 1e-8
B1, B2 = float(torch.tensor(0.9, dtype=F32)), float(torch.tensor(0.999, dtype=F32))
ADAM_CASES = [(1, 1, 1.0, 5.0, 3e-4, 1), (257, 7, 0.25, 5.0, 3e-4, 1000), (92620, 64, 1.0, 5.0, 3e-4, 1), (1000, 4096, 1.0, 0.0, 0.0, 1),
              (255, 1, 1.0, 5.0, 0.0, 1)]


def _adam_ref(p0, m0, v0, grads, gscale, max_norm, wd, step0, dt):
    """-> per step (p, m, v, total norm) from clip_grad_norm_ + torch.optim.Adam in dtype dt"""
    p = torch.nn.Parameter(p0.to(dt).clone())
    opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=ADAM_EPS, weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(float(step0 - 1)), "exp_avg": m0.to(dt).clone(), "exp_avg_sq": v0.to(dt).clone()}
    out = []
    for g in grads:
        p.grad = g.to(dt) * gscale
        if max_norm > 0:
            norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
        else:
            norm = torch.linalg.vector_norm(p.grad)
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), norm.detach().clone()))
    return out


# rule, relative to each quantity's maximum: p 2.4e-7 .. 8.6e-7 (|p| <= 0.1: 2.4e-8 .. 8.6e-8 absolute), m 2.7e-7 .. 5.5e-6, v 4.6e-7 ..
# 1.0e-5, norm 2.4e-7 .. 8.4e-6.  Worst error, emulator = MI355X: p 1.1e-7 (0.13 of the bound), m 2.1e-7 (0.36), v 3.3e-7 (0.42),
# norm 5.4e-8 (0.17)
@pytest.mark.parametrize("n,nblk,gscale,max_norm,wd,step0", ADAM_CASES)
def test_clip_adam(backend, n, nblk, gscale, max_norm, wd, step0):
    ops, dev, name = backend
    p0 = (rnd(900 + n, n) - 0.5) * 0.2
    if step0 > 1:
        m0, v0 = (rnd(901 + n, n) - 0.5) * 0.01, rnd(902 + n, n) * 1e-4
    else:
        m0, v0 = torch.zeros(n), torch.zeros(n)
    # total norms 20, 0.5, 20: clipping (max_norm 5) is active on the first and the third step only
    grads = []
    for k, target in enumerate((20.0, 0.5, 20.0)):
        g = rnd(910 + k + n, n) - 0.5
        grads.append(g * (target / (float(g.double().norm()) * gscale)))
    r64 = _adam_ref(p0, m0, v0, grads, gscale, max_norm, wd, step0, F64)
    r32 = _adam_ref(p0, m0, v0, grads, gscale, max_norm, wd, step0, F32)
    if max_norm > 0:
        assert [float(r[3]) > max_norm for r in r64] == [True, False, True]
    p, m, v = Out(dev, n), Out(dev, n), Out(dev, n)
    p.t.copy_(p0), m.t.copy_(m0), v.t.copy_(v0)
    for k, g in enumerate(grads):
        part, gn = Out(dev, nblk), Out(dev, 1)
        ops.lib.call("zt_clip_adam_f32", p.t, g.to(dev), m.t, v.t, n, part.t, nblk, gscale, max_norm, LR, B1, B2, ADAM_EPS, wd,
                     step0 + k, gn.t, ops._s(p.t))
        part.check()
        for nm, got, i in (("p", p, 0), ("m", m, 1), ("v", v, 2), ("gnorm", gn, 3)):
            check("clip_adam_%s_step%d" % (nm, k), name, got.check(), r64[k][i], r32[k][i])
