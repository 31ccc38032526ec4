"""The fused / tiled kernels of the loss tail against the entry points they replace (bit for bit), the local variance
against a float32 replay of its operation order on the host (bit for bit), and the rewritten 5x5 stencils against the CPU
oracle.  Back-end "emu" runs on the CPU, back-end "hip" (marked gpu) on the MI355X."""
import numpy as np
import pytest
import torch

from test_kernels import _adj_ref, maxerr


def rnd(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


LV_SHAPES = [(5, 6), (16, 64), (17, 65), (37, 131)]      # inside one halo, exactly one tile, ragged second tile, several tiles


@pytest.mark.parametrize("H,W", LV_SHAPES)
def test_localvar_bwd_pair(backend, H, W):
    ops, dev, _ = backend
    DN, DH2, gV, dH3_0 = (rnd(10 + i, 1, 3, H, W).to(dev) for i in range(4))
    ref_dH3 = ops.localvar_bwd(DN, gV, -1.0, out=dH3_0.clone())
    ref_dH2x = ops.localvar_bwd(DH2, gV, 1.0)
    ops.localvar_bwd(DN, gV, 1.0, out=ref_dH2x)
    dH3 = dH3_0.clone()
    dH2x = ops.localvar_bwd_pair(DN, DH2, gV, dH3)
    assert torch.equal(dH3, ref_dH3)
    assert torch.equal(dH2x, ref_dH2x)


@pytest.mark.parametrize("H,W", LV_SHAPES)
def test_localvar_fwd_pair(backend, H, W):
    ops, dev, _ = backend
    H2, H3 = rnd(20, 1, 3, H, W).to(dev), rnd(21, 1, 3, H, W).to(dev)
    rDH2, rVH2 = ops.localvar_fwd(H2)
    rDN, rVN = ops.localvar_fwd(H3, H2)
    DH2, VH2, DN, VN = ops.localvar_fwd_pair(H2, H3)
    for got, ref in ((DH2, rDH2), (VH2, rVH2), (DN, rDN), (VN, rVN)):
        assert torch.equal(got, ref)


def _box0(x):
    """zero-padded 5x5 box sum in float32: row sums left to right, then column sums top to bottom"""
    H, W = x.shape[-2:]
    q = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)])
    hs = (((q[..., 0:W] + q[..., 1:W + 1]) + q[..., 2:W + 2]) + q[..., 3:W + 3]) + q[..., 4:W + 4]
    return (((hs[..., 0:H, :] + hs[..., 1:H + 1, :]) + hs[..., 2:H + 2, :]) + hs[..., 3:H + 3, :]) + hs[..., 4:H + 4, :]


def _lv_fwd_host(a, b=None):
    f25 = np.float32(25)
    x = a if b is None else a - b
    D = x - _box0(x) / f25
    return D, _box0(D * D) / f25


def _lv_bwd_host(D, gV, sign):
    f25 = np.float32(25)
    S = _box0(gV) / f25
    E = np.float32(2) * D * S
    return np.float32(sign) * (E - _box0(E) / f25)


@pytest.mark.parametrize("H,W", LV_SHAPES)
def test_localvar_host_replay(backend, H, W):
    """The single and the pair entry points are instantiations of one kernel template, so the pair tests above compare a text
    with itself; this numpy float32 replay of the documented operation order anchors the arithmetic, bit for bit."""
    ops, dev, _ = backend
    ta, tb, tD2, tgV, tacc = (rnd(120 + i, 1, 3, H, W) for i in range(5))
    a, b, D2, gV, acc = (t.numpy() for t in (ta, tb, tD2, tgV, tacc))
    assert a.dtype == np.float32

    def same(got, ref):
        assert ref.dtype == np.float32
        assert np.array_equal(got.cpu().numpy(), ref)

    rDa, rVa = _lv_fwd_host(a)
    rDx, rVx = _lv_fwd_host(b, a)
    da, db = ta.to(dev), tb.to(dev)
    D, V = ops.localvar_fwd(da)
    same(D, rDa), same(V, rVa)
    D, V = ops.localvar_fwd(db, da)
    same(D, rDx), same(V, rVx)
    none, V = ops.localvar_fwd(da, want_D=False)                     # null D
    assert none is None
    same(V, rVa)
    for got, ref in zip(ops.localvar_fwd_pair(da, db), (rDa, rVa, rDx, rVx)):
        same(got, ref)

    dD, dD2, dgV = torch.from_numpy(rDa).to(dev), tD2.to(dev), tgV.to(dev)
    same(ops.localvar_bwd(dD, dgV, 1.0), _lv_bwd_host(rDa, gV, 1))
    same(ops.localvar_bwd(dD2, dgV, -1.0), _lv_bwd_host(D2, gV, -1))
    same(ops.localvar_bwd(dD2, dgV, -1.0, out=tacc.clone().to(dev)), acc + _lv_bwd_host(D2, gV, -1))
    dH3 = tacc.clone().to(dev)
    dH2x = ops.localvar_bwd_pair(dD2, dD, dgV, dH3)                  # DN = D2, DH2 = D
    same(dH3, acc + _lv_bwd_host(D2, gV, -1))
    same(dH2x, _lv_bwd_host(rDa, gV, 1) + _lv_bwd_host(D2, gV, 1))


HALF_SHAPES = [(6, 7), (9, 70), (20, 28), (21, 133)]
HALF_CASES = [(h, w, 2 * h, 2 * w) for h, w in HALF_SHAPES] + [(h, w, 2 * h + 1, 2 * w + 1) for h, w in HALF_SHAPES[:2]]


@pytest.mark.parametrize("h,w,H,W", HALF_CASES)
def test_half_bwd(backend, h, w, H, W):
    ops, dev, _ = backend
    u1, u2, g1, g2 = (rnd(30 + i, 1, 3, h, w).to(dev) for i in range(4))
    r1 = ops.box5_reflect_adj(u1, -1.0, out=g1.clone())
    r2 = ops.box5_reflect_adj(u2, -1.0, out=g2.clone())
    ref = ops.pair_down_adj(r1, r2, H, W)
    k1, k2 = g1.clone(), g2.clone()
    got = torch.full((1, 3, H, W), float("nan"), device=dev)        # every element must be written, the zero fringe included
    ops.lib.call("zt_half_bwd_f32", u1, u2, g1, g2, got, 3, H, W, ops._s(u1))
    assert torch.equal(got, ref)
    assert torch.equal(ops.half_bwd(u1, u2, g1, g2, H, W), ref)
    assert torch.equal(g1, k1) and torch.equal(g2, k2)             # the half-resolution gradients are not written back


@pytest.mark.parametrize("H,W", HALF_SHAPES)
def test_box5_reflect_tiled(backend, oracle, H, W):
    """tolerances of test_kernels.py::test_stencils"""
    ops, dev, _ = backend
    x, g = rnd(40, 1, 3, H, W), rnd(41, 1, 3, H, W)
    assert maxerr(ops.box5_reflect(x.to(dev)), oracle.local_mean_reflect(x)) < 1e-6
    ref = _adj_ref(oracle.local_mean_reflect, x, g)
    assert maxerr(ops.box5_reflect_adj(g.to(dev), 1.0), ref) < 1e-6
    acc0 = rnd(42, 1, 3, H, W)
    assert maxerr(ops.box5_reflect_adj(g.to(dev), -1.0, out=acc0.clone().to(dev)), acc0 - ref) < 1e-6


@pytest.mark.parametrize("H,W", HALF_SHAPES)
def test_texture_mask_tiled(backend, oracle, H, W):
    """tolerances of test_kernels.py::test_stencils: ratio within 2e-5, at most 1e-3 of the mask elements differ"""
    ops, dev, _ = backend
    a, b = rnd(50, 1, 3, H, W), rnd(51, 1, 3, H, W)
    m, r = ops.texture_mask(a.to(dev), b.to(dev), want_ratio=True)
    rm, rr = oracle.texture_mask(a, b)
    assert maxerr(r, rr) < 2e-5
    assert (m.cpu() != rm).float().mean().item() <= 1e-3
    assert torch.equal(ops.texture_mask(a.to(dev), b.to(dev)), m)


# ---------------------------------------------------------------------------------------------------- NHWC emitters
EMIT_SHAPES = [(4, 6), (10, 22), (36, 264)]                   # the last one: W/2 = 132 spans three 64-wide blocks, ragged


def _bf16_buf(dev, npix, off_bytes):
    """[npix, 8] bf16 view whose base pointer is 16-byte aligned plus off_bytes"""
    raw = torch.full((npix * 8 + 8,), float("nan"), dtype=torch.bfloat16, device=dev)
    assert raw.data_ptr() % 16 == 0
    v = raw[off_bytes // 2: off_bytes // 2 + npix * 8].view(npix, 8)
    assert v.data_ptr() % 16 == off_bytes
    return v


def _check_bf16(got, ref32, nch):
    """bf16 ld = 8 output == fp32 reference rounded to bf16, pad channels exactly zero"""
    assert torch.equal(got[:, :nch].cpu(), ref32[:, :nch].cpu().to(torch.bfloat16))
    assert torch.equal(got[:, nch:].cpu(), torch.zeros_like(got[:, nch:].cpu()))


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("H,W", EMIT_SHAPES)
def test_clamp_sub6_bwd_bf16(backend, H, W, off):
    ops, dev, _ = backend
    HW = H * W
    A, B = rnd(60, 1, 3, H, W).to(dev), rnd(61, 1, 3, H, W).to(dev)
    r = (rnd(62, 1, 6, H, W) * 1.2 - 0.3).to(dev)                    # A - r leaves [1e-4, 1] on both sides
    gA, gB = (rnd(63, 1, 3, H, W) - 0.5).to(dev), (rnd(64, 1, 3, H, W) - 0.5).to(dev)
    # reference: fp32 output; six channels need ld >= 6, so the fp32 call uses ld = 8 (scalar path)
    ref = torch.full((HW, 8), float("nan"), device=dev)
    ops.lib.call("zt_clamp_sub6_bwd", A, B, r, gA, gB, ref, 0, 8, HW, ops._s(A))
    got = _bf16_buf(dev, HW, off)
    ops.lib.call("zt_clamp_sub6_bwd", A, B, r, gA, gB, got, 1, 8, HW, ops._s(A))
    _check_bf16(got, ref, 6)


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("H,W", EMIT_SHAPES)
def test_post_enh_bwd_bf16(backend, H, W, off):
    ops, dev, _ = backend
    h, w = H // 2, W // 2
    x = (rnd(70, 1, 3, H, W) * 0.8).to(dev)
    s2 = rnd(71, 1, 3, H, W)
    s2[s2 < 0.05] = 1e-4                                             # the Enhancer's clamp floor: dO = 0 there
    s2 = s2.to(dev)
    L11, L12 = (rnd(72, 1, 3, h, w) * 0.8).to(dev), (rnd(73, 1, 3, h, w) * 0.8).to(dev)
    s21, s22 = (rnd(74, 1, 3, h, w) * 0.9 + 0.1).to(dev), (rnd(75, 1, 3, h, w) * 0.9 + 0.1).to(dev)
    dIn5, dH2x = (rnd(76, 1, 12, H, W) - 0.5).to(dev), (rnd(77, 1, 3, H, W) - 0.5).to(dev)
    dIn3, dIn4 = (rnd(78, 1, 12, h, w) - 0.5).to(dev), (rnd(79, 1, 12, h, w) - 0.5).to(dev)
    ds2 = (rnd(80, 1, 3, H, W) - 0.5).to(dev)
    s = ops._s(x)
    ref, tot_ref = torch.full((H * W, 4), float("nan"), device=dev), torch.empty(1, 3, H, W, device=dev)
    ops.lib.call("zt_post_enh_bwd", x, s2, L11, L12, s21, s22, dIn5, dH2x, dIn3, dIn4, ds2, ref, 0, 4, tot_ref, H, W, s)
    got, tot = _bf16_buf(dev, H * W, off), torch.empty(1, 3, H, W, device=dev)
    ops.lib.call("zt_post_enh_bwd", x, s2, L11, L12, s21, s22, dIn5, dH2x, dIn3, dIn4, ds2, got, 1, 8, tot, H, W, s)
    _check_bf16(got, ref, 3)
    assert torch.equal(ref[:, 3].cpu(), torch.zeros(H * W))
    assert torch.equal(tot, tot_ref)
    got2 = _bf16_buf(dev, H * W, off)
    ops.lib.call("zt_post_enh_bwd", x, s2, L11, L12, s21, s22, dIn5, dH2x, dIn3, dIn4, ds2, got2, 1, 8, None, H, W, s)
    assert torch.equal(got2.cpu(), got.cpu())                        # the engine's call: no ds2_total


@pytest.mark.parametrize("off", [0, 8])
@pytest.mark.parametrize("H,W", EMIT_SHAPES)
def test_d1_bwd_prep_bf16(backend, H, W, off):
    ops, dev, _ = backend
    h, w = H // 2, W // 2
    x, n = rnd(90, 1, 3, H, W).to(dev), (rnd(91, 1, 3, H, W) * 1.2 - 0.3).to(dev)
    dLp1, dLp2, dden1, dden2 = ((rnd(92 + i, 1, 3, h, w) - 0.5).to(dev) for i in range(4))
    s = ops._s(x)
    refs = [torch.full((H * W, 4), float("nan"), device=dev)] + [torch.full((h * w, 4), float("nan"), device=dev) for _ in range(2)]
    ops.lib.call("zt_d1_bwd_prep", x, n, dLp1, dLp2, dden1, dden2, refs[0], refs[1], refs[2], 0, 4, H, W, s)
    gots = [_bf16_buf(dev, H * W, off), _bf16_buf(dev, h * w, off), _bf16_buf(dev, h * w, off)]
    ops.lib.call("zt_d1_bwd_prep", x, n, dLp1, dLp2, dden1, dden2, gots[0], gots[1], gots[2], 1, 8, H, W, s)
    for got, ref in zip(gots, refs):
        _check_bf16(got, ref, 3)


# ---------------------------------------------------------------------------------------------------- scalars and reductions
NBLKS = [1, 3, 256, 300]
SCALAR_NBLKS = NBLKS + [700]                                  # 300 and 700: two and three LDS chunks of 256 partial rows


def _partials(seed, *shape):
    """positive partial sums spanning 1e-6 .. 1e3"""
    return torch.pow(10.0, rnd(seed, *shape) * 9.0 - 6.0)


def _scalar_case(nblk):
    """partials [nblk][3] and a pixel count HW for which every channel mean lies in 0.03 .. 0.25, so that no enhancement
    factor reaches its clamp (1 or 25) and every output depends on the sums.  A channel outside that range is moved to a mean
    of 0.05 .. 0.1 by a power of two, which keeps its values' relative spread."""
    part = _partials(100 + nblk, nblk, 3)
    sums = part.double().sum(0)
    HW = max(4, int(float(sums.max()) / 0.2))
    for c in range(3):
        mean = float(sums[c]) / HW
        if not 0.03 <= mean <= 0.25:
            part[:, c] *= 2.0 ** int(np.floor(np.log2(0.1 / mean)))
    return part, HW


@pytest.mark.parametrize("is_WB", [0, 1])
@pytest.mark.parametrize("nblk", SCALAR_NBLKS)
def test_loss_scalars(backend, nblk, is_WB):
    """against zt_loss_scalars_serial_f32, the one-lane definition: same additions in the same order, bit for bit"""
    ops, dev, _ = backend
    part, HW = _scalar_case(nblk)
    part = part.to(dev)
    got, ref = torch.full((8,), float("nan"), device=dev), torch.full((8,), float("nan"), device=dev)
    ops.lib.call("zt_loss_scalars_serial_f32", part, nblk, HW, is_WB, ref, ops._s(part))
    ops.lib.call("zt_loss_scalars_f32", part, nblk, HW, is_WB, got, ops._s(part))
    e = ref[:3].cpu()
    assert bool(((e > 1.0) & (e < 25.0)).all()), e                   # un-clamped: the outputs depend on the sums
    assert torch.equal(got[:6], ref[:6])
    # the sums themselves, replayed on the host in fp64 (python floats) and fp32 (numpy): exact for the un-clamped factors
    pc = part.cpu()
    s = [0.0, 0.0, 0.0]
    for b in range(nblk):
        for c in range(3):
            s[c] += float(pc[b, c])
    f32 = np.float32
    if is_WB:
        ef = [f32(0.3) / (f32(s[c] / float(HW)) + f32(1e-9)) for c in range(3)]
    else:
        ef = [f32(0.5) / (f32((0.299 * s[2] + 0.587 * s[1] + 0.144 * s[0]) / float(HW)) + f32(1e-9))] * 3
    assert np.array_equal(e.numpy(), np.array(ef, dtype=np.float32))


def _column_sum_host(col):
    """partial_reduce_kernel's summation on the host: thread t adds rows t, t + 256, ... in fp64, then the 128 -> 1 tree"""
    col = col.double().numpy()
    sh = np.zeros(256)
    for t in range(min(256, len(col))):
        acc = 0.0
        for v in col[t::256]:
            acc += float(v)
        sh[t] = acc
    w = 128
    while w > 0:
        sh[:w] = sh[:w] + sh[w:2 * w]
        w >>= 1
    return np.float32(sh[0])


@pytest.mark.parametrize("nblk", NBLKS)
def test_loss_terms_reduce(backend, nblk):
    ops, dev, _ = backend
    nb1, nb2, nb3 = nblk, nblk + 1, 2 * nblk + 5
    c1, c2, c3 = _partials(110, nb1, 4), _partials(111, nb2, 10), _partials(112, nb3, 3)
    p1, p2, p3 = c1.to(dev), c2.to(dev), c3.to(dev)
    s = ops._s(p1)
    ref = torch.full((17,), float("nan"), device=dev)
    ops.partial_reduce(p1, nb1, 4, 4, out=ref)
    ops.lib.call("zt_partial_reduce_f32", p2, nb2, 10, 8, ref.data_ptr() + 16, 0, None, s)
    ops.lib.call("zt_partial_reduce_f32", p2.data_ptr() + 32, nb2, 10, 2, ref.data_ptr() + 56, 0, None, s)
    ops.lib.call("zt_partial_reduce_f32", p3, nb3, 3, 2, ref.data_ptr() + 48, 0, None, s)
    ops.lib.call("zt_partial_reduce_f32", p3.data_ptr() + 8, nb3, 3, 1, ref.data_ptr() + 64, 0, None, s)
    got = torch.full((17,), float("nan"), device=dev)
    ops.loss_terms_reduce(p1, nb1, p2, nb2, p3, nb3, got)
    assert torch.equal(got, ref)
    # both launches share one summation routine: hold it to the same fixed-order fp64 sum replayed on the host
    cols = [c1[:, j] for j in range(4)] + [c2[:, j] for j in range(8)] + [c3[:, 0], c3[:, 1], c2[:, 8], c2[:, 9], c3[:, 2]]
    host = np.array([_column_sum_host(c) for c in cols], dtype=np.float32)
    assert np.array_equal(got.cpu().numpy(), host)
