"""The on-the-fly correlation path (zt_corr_alt.hip, `RaftPlan(alternate_corr=True)`): the 4 x 81 window of the lookup
computed from the two feature maps, never forming the all-pairs volume.

1. integer operands: every partial sum of every level is exact in fp32, so `fmap_pyramid` + `corr_alt_lookup` must be the bits of
   `corr_pyramid` + `corr_lookup` on the exact volume -- tap order, channel order, the floor at odd sizes, the window position and
   the clamp all show here;
2. random operands against a float64 restatement and against the oracle's pooled-volume definition, under a bound the test
   computes from the operands;
3. the step form (flow bookkeeping folded in) against `zt_raft_flow_step` + the plain call, bit for bit;
4. the two plans on the same frames: first-iteration CORR and the final flow;  5. peak memory;  6. graph replay;  7. the scripts.

Every figure is printed before it is asserted ("CORRALT ..." lines, visible with -s)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import frames

SENT = -768.0            # exact in bf16 and fp32; no kernel under test produces it
MAPS = [(16, 16), (17, 21), (16, 19), (23, 18)]      # the smallest legal map + three where every level drops a row or a column
ALPHA = 1.0 / 16.0
LDF = 264                # feature pitch > 256 (a multiple of 8): the padding channels hold NaN and must never be read
U24 = 2.0 ** -24


def _stream(dev):
    return importlib.import_module("zero-tig_amd.lib").current_stream(dev)


def _below(v):
    return float(torch.nextafter(torch.tensor(v), torch.tensor(-float("inf"))))


_cases = {}


def _coords_case(h, w):
    """the pixel grid + 3 * randn with the planted cases of test_raft_loop._corr_case, a half-integer pair and negative / positive
    coordinates one ulp below an integer; computed once per map, never written"""
    if (h, w) not in _cases:
        g = torch.Generator().manual_seed(h * 100 + w)
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        grid = torch.stack([xs, ys], -1).float().reshape(-1, 2)
        flat = grid + 3.0 * torch.randn(h * w, 2, generator=g)
        planted = [(w - 1.0, h - 1.0), (float(w), float(h)), (-1.0, -1.0), (3.0, 2.0), (-50.0, -50.0), (1e6, 3.0), (-1e9, 1e9),
                   (5.5, 7.5), (_below(-1.0), _below(0.0)), (_below(4.0), _below(-2.0)), (_below(0.0), 6.25)]
        where = [5 + 23 * i for i in range(len(planted))]       # 5 + 23 * 10 = 235 < 16 * 16
        for n, p in zip(where, planted):
            flat[n] = torch.tensor(p)
        _cases[(h, w)] = dict(coords=flat.contiguous(), grid=grid.contiguous(), far=where[4:7])
    return _cases[(h, w)]


def _store(f, adt, dev):
    """[npx][256] values -> a [npx][LDF] buffer of the storage type with NaN in the padding channels; returns the 256-wide view's
    parent so that shape[-1] is the pitch"""
    buf = torch.full((f.shape[0], LDF), float("nan"), dtype=adt)
    buf[:, :256] = f.to(adt)
    return buf.to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against the volume path, integer operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "%dx%d" % s)
def test_alt_lookup_equals_volume_lookup_integer_operands(backend, hw, store):
    """f1, f2 integers in [-3, 3]: |dot| <= 2304, level-3 features are multiples of 1/64, alpha * dot multiples of 1/1024 below 144
    (18 bits) -- summation order and the two ways of pooling cannot differ, so torch.equal is the contract."""
    ops, dev, _ = backend
    h, w = hw
    npx = h * w
    c = _coords_case(h, w)
    g = torch.Generator().manual_seed(7 * h + w)
    f1 = torch.randint(-3, 4, (npx, 256), generator=g).float()
    f2 = torch.randint(-3, 4, (npx, 256), generator=g).float()
    # the volume path on the exact products
    pitch = (npx + 15) // 16 * 16
    c0 = torch.full((1, h, w, pitch), float("nan"))
    c0[0, :, :, :npx] = ((f1.double() @ f2.double().t()) * ALPHA).float().view(h, w, npx)
    c0 = c0.to(dev)
    coords = c["coords"].to(dev)
    levels = ops.corr_pyramid(c0, h, w)
    adt = torch.bfloat16 if store == "bf16" else torch.float32
    F1, F2 = _store(f1, adt, dev), _store(f2, adt, dev)
    pyr = ops.fmap_pyramid(F2, h, w)
    # the pooled features themselves: avg_pool2d with floor sizes, exact here
    P = f2.view(1, h, w, 256).permute(0, 3, 1, 2)
    for lv in pyr:
        P = F.avg_pool2d(P, 2, stride=2)
        assert tuple(lv.shape) == (P.shape[2] * P.shape[3], 256)
        assert torch.equal(lv.cpu(), P[0].permute(1, 2, 0).reshape(-1, 256))
    for odt in (torch.float32, torch.bfloat16):
        ref = torch.full((1, h, w, 328), SENT, dtype=odt, device=dev)
        ops.corr_lookup(c0, levels, h, w, coords, out=ref)
        out = torch.full((1, h, w, 328), SENT, dtype=odt, device=dev)
        ops.corr_alt_lookup(F1, F2, pyr, h, w, coords, out=out)
        bad = (out[..., :324] != ref[..., :324]).sum()
        print("CORRALT exact [%dx%d store %s out %s] differing elements %d" % (h, w, store, str(odt)[6:], int(bad)))
        assert torch.equal(out[..., :324], ref[..., :324])
        assert bool((out[..., 324:] == SENT).all()) and not bool((out[..., :324] == SENT).any())
        far = out.view(npx, 328)[c["far"], :324].float()
        assert far.shape == (3, 324) and bool(torch.isfinite(far).all()) and bool((far == 0).all())
    assert torch.equal(coords.cpu(), c["coords"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. random floats against fp64
# ---------------------------------------------------------------------------------------------------------------------
def _taps32(p, l, size):
    """corr_lookup_kernel's coordinate sequence for the nine window positions of one axis, in fp32 as the kernel does it (every
    operation is a single IEEE operation in both): -> (tap index int64 [n, 9] after the clamp, weight of the second tap fp32)"""
    i = torch.arange(9, dtype=torch.float32) - 4.0
    c = p[:, None] / float(1 << l) + i[None]
    gx = 2.0 * c / float(size - 1) - 1.0
    ic = (gx + 1.0) * torch.tensor((size - 1) / 2.0, dtype=torch.float32)
    f0 = torch.floor(ic)
    w1 = ic - f0
    return torch.clamp(f0, -2.0, size + 1.0).long(), w1


def _restate(f1, f2, h, w, coords):
    """float64 restatement: pooled fmap2 (each level from the level below, nothing rounded), dots at the integer grid, the bilinear
    rule with zeros outside.  -> (value, S, level) per output element [npx, 324]; S is the same bilinear combination of
    sum_c |f1_c| |P_l,c|, weights in absolute value."""
    npx = h * w
    f1 = f1.double()
    P = f2.double().view(1, h, w, 256).permute(0, 3, 1, 2)
    val, S, lvl = [], [], []
    for l in range(4):
        if l:
            P = F.avg_pool2d(P, 2, stride=2)
        hl, wl = P.shape[2:]
        Pm = P[0].permute(1, 2, 0).reshape(-1, 256)
        Dm, Sm = (f1 @ Pm.t()) * ALPHA, (f1.abs() @ Pm.abs().t()) * ALPHA          # dots at every integer point of the level
        x0, wx1 = _taps32(coords[:, 0], l, wl)
        y0, wy1 = _taps32(coords[:, 1], l, hl)
        wx0, wy0 = 1.0 - wx1, 1.0 - wy1                                              # fp32, as the kernel
        v, s = torch.zeros(npx, 9, 9, dtype=torch.float64), torch.zeros(npx, 9, 9, dtype=torch.float64)
        for dx, dy, wx, wy in ((0, 0, wx0, wy0), (1, 0, wx1, wy0), (0, 1, wx0, wy1), (1, 1, wx1, wy1)):
            xx, yy = (x0 + dx)[:, :, None].expand(npx, 9, 9), (y0 + dy)[:, None, :].expand(npx, 9, 9)
            ok = (xx >= 0) & (xx < wl) & (yy >= 0) & (yy < hl)
            idx = (yy.clamp(0, hl - 1) * wl + xx.clamp(0, wl - 1)).reshape(npx, 81)
            wgt = (wx[:, :, None] * wy[:, None, :]).double()                         # the fp32 product the kernel forms
            wgt = torch.where(ok, wgt, torch.zeros_like(wgt))
            v += torch.nan_to_num(wgt) * torch.gather(Dm, 1, idx).view(npx, 9, 9)
            s += torch.nan_to_num(wgt).abs() * torch.gather(Sm, 1, idx).view(npx, 9, 9)
        val.append(v.reshape(npx, 81))                                               # [n][i*9 + j], i moving x
        S.append(s.reshape(npx, 81))
        lvl.append(torch.full((npx, 81), float(l), dtype=torch.float64))
    return torch.cat(val, 1), torch.cat(S, 1), torch.cat(lvl, 1)


def _bound(S, lvl, ref, bf16_out):
    """(256 + 16) * 2^-24 * alpha * S (256 additions of the dot, 16 for the bilinear combination) + the fp32 rounding of P_l
    (3 * 2^-24 relative per level) + half a bf16 ulp of the value for bf16 outputs (2^-8 relative covers it).  alpha is in S."""
    b = (256 + 16) * U24 * S + 3 * U24 * lvl * S
    return b + ref.abs() * 2.0 ** -8 if bf16_out else b


@pytest.mark.parametrize("store", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "%dx%d" % s)
def test_alt_lookup_random_against_fp64(backend, oracle, hw, store):
    ops, dev, _ = backend
    h, w = hw
    npx = h * w
    c = _coords_case(h, w)
    g = torch.Generator().manual_seed(11 * h + w)
    adt = torch.bfloat16 if store == "bf16" else torch.float32
    f1 = torch.randn(npx, 256, generator=g).to(adt).float()                          # the values the kernels see
    f2 = torch.randn(npx, 256, generator=g).to(adt).float()
    F1, F2 = _store(f1, adt, dev), _store(f2, adt, dev)
    coords = c["coords"].to(dev)
    pyr = ops.fmap_pyramid(F2, h, w)
    ref, S, lvl = _restate(f1, f2, h, w, c["coords"])
    nchw = lambda t: t.t().reshape(1, 256, h, w).contiguous()
    cmap = c["coords"].view(h, w, 2).permute(2, 0, 1)[None].contiguous()
    orc = oracle.corr_lookup(oracle.corr_pyramid(nchw(f1), nchw(f2)), cmap).permute(0, 2, 3, 1).reshape(npx, 324).double()
    for odt in (torch.float32, torch.bfloat16):
        out = torch.full((1, h, w, 328), SENT, dtype=odt, device=dev)
        ops.corr_alt_lookup(F1, F2, pyr, h, w, coords, out=out)
        got = out.view(npx, 328)[:, :324].double().cpu()
        assert bool(torch.isfinite(got).all()) and bool((out[..., 324:] == SENT).all())
        bound = _bound(S, lvl, ref, odt == torch.bfloat16)
        for name, r in (("fp64", ref), ("oracle", orc)):
            err = (got - r).abs()
            worst = float((err - bound).max())
            print("CORRALT random [%dx%d store %s out %s] vs %s: max err %.3e, max (err - bound) %.3e, max err/bound %.3f"
                  % (h, w, store, str(odt)[6:], name, float(err.max()), worst, float((err / bound.clamp_min(1e-30)).max())))
            assert bool((err <= bound).all()), (name, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the step form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "%dx%d" % s)
def test_alt_lookup_step_equals_flow_step_then_lookup(backend, hw, dt):
    ops, dev, _ = backend
    lib, s = ops.lib, _stream(dev)
    h, w = hw
    npx = h * w
    c = _coords_case(h, w)
    adt, ldfin, ldo = (torch.bfloat16, 8, 328) if dt else (torch.float32, 4, 324)
    es = 2 if dt else 4
    g = torch.Generator().manual_seed(npx + dt)
    F1, F2 = _store(torch.randn(npx, 256, generator=g), adt, dev), _store(torch.randn(npx, 256, generator=g), adt, dev)
    pyr = ops.fmap_pyramid(F2, h, w)
    delta = torch.randn(npx, 4, generator=g)
    delta[:, 2:] = float("nan")                                 # only the first two columns are the flow update
    delta = delta.to(dev)
    coords = c["coords"].to(dev)

    def buffers():
        f = lambda *shape, dtype=adt: torch.full(shape, SENT, dtype=dtype, device=dev)
        return dict(F4=f(1, h, w, 4, dtype=torch.float32), HX=f(1, h, w, 384), FIN=f(1, h, w, ldfin), CORR=f(1, h, w, ldo))
    A, B = buffers(), buffers()
    coordsA = coords.clone()
    lib.call("zt_raft_flow_step", coordsA, delta, 4, h, w, A["F4"], 4, A["HX"].data_ptr() + es * 382, 384, A["FIN"], ldfin, dt, s)
    ops.corr_alt_lookup(F1, F2, pyr, h, w, coordsA, out=A["CORR"])
    coordsB = torch.full((npx, 2), SENT, dtype=torch.float32, device=dev)
    ops.corr_alt_lookup_step(F1, F2, pyr, h, w, coords, B["CORR"], delta, coordsB, B["F4"], B["HX"].data_ptr() + es * 382, 384, B["FIN"])
    assert torch.equal(coords.cpu(), c["coords"])               # the fused launch reads its coordinates only
    assert torch.equal(coordsB, coordsA) and torch.equal(coordsB, coords + delta[:, :2])
    for k in ("F4", "HX", "FIN", "CORR"):
        assert torch.equal(A[k], B[k]), k
    flow = coordsB - c["grid"].to(dev)
    assert torch.equal(B["F4"][..., :2].reshape(npx, 2), flow) and bool((B["F4"][..., 2:] == SENT).all())
    assert torch.equal(B["HX"][..., 382:].reshape(npx, 2), flow.to(adt)) and bool((B["HX"][..., :382] == SENT).all())
    assert torch.equal(B["FIN"][..., :2].reshape(npx, 2), flow.to(adt)) and bool((B["FIN"][..., 2:] == SENT).all())
    assert not bool((B["CORR"][..., :324] == SENT).any()) and bool((B["CORR"][..., 324:] == SENT).all())
    # the launcher refuses to alias its two coordinate buffers, and a delta that would not be recorded
    for cout in (coords, None):
        with pytest.raises(RuntimeError, match="1001"):
            ops.corr_alt_lookup_step(F1, F2, pyr, h, w, coords, B["CORR"], delta, cout, B["F4"], B["HX"].data_ptr() + es * 382, 384, B["FIN"])
    assert torch.equal(A["CORR"], B["CORR"]) and torch.equal(coords.cpu(), c["coords"])


def test_alt_entry_points_reject_small_maps(backend):
    """h, w >= 16 as for the volume: a level of one pixel divides by W - 1 = 0"""
    ops, dev, _ = backend
    h, w = 16, 15
    f = torch.zeros(h * w, 256, device=dev)
    with pytest.raises(RuntimeError, match="1001"):
        ops.fmap_pyramid(f, h, w)
    pyr = [torch.zeros(64, 256, device=dev) for _ in range(3)]
    out = torch.full((1, h, w, 324), SENT, device=dev)
    with pytest.raises(RuntimeError, match="1001"):
        ops.corr_alt_lookup(f, f, pyr, h, w, torch.zeros(h * w, 2, device=dev), out=out)
    assert bool((out == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the plan: RaftPlan(alternate_corr=True) against RaftPlan() on the same frames
# ---------------------------------------------------------------------------------------------------------------------
def _raft_weights(synth, dev, seed=3):
    st = synth.make_state(seed)
    return st, {k: torch.from_numpy(np.array(v)).to(dev) for k, v in st.items() if k.startswith("raft.")}


def _pair(synth, H, W, dev):
    """two consecutive frames of the synthetic clip's clean twin, [1,3,H,W] in [0, 255]"""
    f = lambda t: torch.from_numpy(np.ascontiguousarray(np.asarray(synth.clean_frame(t, H, W, 2), dtype=np.float32).reshape(1, 3, H, W)))
    return (f(0) * 255.0).to(dev).contiguous(), (f(1) * 255.0).to(dev).contiguous()


def _pack(ops, a, b, bf, dev):
    H, W = a.shape[-2:]
    x2 = torch.empty((2, H, W, 8 if bf else 4), dtype=torch.bfloat16 if bf else torch.float32, device=dev)
    ops.lib.call("zt_raft_pack_pair", a, b, x2, int(bf), x2.shape[-1], H, W, H, W, _stream(dev))
    return x2


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(128, 128), (136, 184)], ids=lambda s: "%dx%d" % s)
def test_plan_alternate_corr_against_volume_plan(hip_ops, oracle, synth, size, precision):
    """Maps 16 x 16 and 17 x 23.  First-iteration CORR of the two plans: within the bound of test 2 evaluated on the plan's own
    feature maps (fp32); in bf16 mode both sides are their fp32 value rounded to bf16, so half a bf16 ulp is allowed for each side.
    flow_up after 12 iterations against the oracle's RAFT.forward (oracle.raft_forward, torch in fp32: the oracle has no float64
    RAFT for raw frames -- its lookup and feature maps are cast to float): the alt plan's maximum error is at most twice the volume
    plan's, both being draws of the same rounding noise amplified by the same loop."""
    ops, dev = hip_ops
    raft = importlib.import_module("zero-tig_amd.raft")
    H, W = size
    h, w = H // 8, W // 8
    npx = h * w
    bf = precision == "bf16"
    st, Wd = _raft_weights(synth, dev)
    a, b = _pair(synth, H, W, dev)
    x2 = _pack(ops, a, b, bf, dev)
    res = {}
    for alt in (False, True):
        plan = raft.RaftPlan(ops, Wd, dev, precision=precision, alternate_corr=alt)
        n0 = {k: ops.lib.calls.get(k, 0) for k in ("zt_corr_lookup", "zt_corr_lookup_step", "zt_corr_alt_lookup", "zt_corr_alt_lookup_step")}
        low, up, aux = plan.run(x2, iters=12, want_aux=True)
        n = {k: ops.lib.calls.get(k, 0) - v for k, v in n0.items()}
        assert n == ({"zt_corr_lookup": 0, "zt_corr_lookup_step": 0, "zt_corr_alt_lookup": 1, "zt_corr_alt_lookup_step": 11} if alt else
                     {"zt_corr_lookup": 1, "zt_corr_lookup_step": 11, "zt_corr_alt_lookup": 0, "zt_corr_alt_lookup_step": 0}), n
        res[alt] = (low.cpu(), up.cpu(), aux)
    f1 = res[True][2]["fmap1"].float().cpu().view(npx, 256)
    f2 = res[True][2]["fmap2"].float().cpu().view(npx, 256)
    grid = _coords_case(16, 16)["grid"] if (h, w) == (16, 16) else None
    if grid is None:
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        grid = torch.stack([xs, ys], -1).float().reshape(-1, 2)
    ref, S, lvl = _restate(f1, f2, h, w, grid)
    ca, cv = (res[k][2]["corr0"].view(npx, -1)[:, :324].double().cpu() for k in (True, False))
    bound = _bound(S, lvl, ref, False)
    if bf:
        bound = bound + (ca.abs() + cv.abs()) * 2.0 ** -8
    err = (ca - cv).abs()
    print("CORRALT plan [%dx%d %s] CORR alt vs volume: max |diff| %.3e, max diff/bound %.3f; alt vs fp64 restatement %.3e"
          % (H, W, precision, float(err.max()), float((err / bound.clamp_min(1e-30)).max()), float((ca - ref).abs().max())))
    assert bool((err <= bound).all())
    with torch.no_grad():
        _, up_o = oracle.raft_forward(oracle.to_torch_state(st), a.cpu(), b.cpu(), iters=12)
    e_alt, e_vol = float((res[True][1] - up_o).abs().max()), float((res[False][1] - up_o).abs().max())
    print("CORRALT plan [%dx%d %s] flow_up vs oracle: alt %.3e, volume %.3e, alt vs volume %.3e, max |flow| %.2f"
          % (H, W, precision, e_alt, e_vol, float((res[True][1] - res[False][1]).abs().max()), float(up_o.abs().max())))
    assert e_alt <= 2.0 * e_vol, (e_alt, e_vol)


# ---------------------------------------------------------------------------------------------------------------------
# 5. memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plan_alternate_corr_peak_memory(hip_ops, synth):
    """512 x 512, map 64 x 64: level 0 of the volume alone is 4096^2 * 4 B = 67 MB; the on-the-fly plan's peak over run() is lower by
    at least 0.9 of that, and its state holds no volume"""
    ops, dev = hip_ops
    raft = importlib.import_module("zero-tig_amd.raft")
    _, Wd = _raft_weights(synth, dev)
    a, b = _pair(synth, 512, 512, dev)
    x2 = _pack(ops, a, b, True, dev)
    peak, states = {}, {}
    for alt in (False, True):
        plan = raft.RaftPlan(ops, Wd, dev, precision="bf16", alternate_corr=alt)
        made, new_state = [], plan.new_state
        plan.new_state = lambda *args, **kw: (made.append(new_state(*args, **kw)), made[-1])[1]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = plan.run(x2, iters=2)
        torch.cuda.synchronize()
        peak[alt] = torch.cuda.max_memory_allocated(dev) - base
        states[alt] = made[0]
        del out, plan
    vol0 = 4096 * 4096 * 4
    print("CORRALT memory [512x512 bf16] peak over run(): volume %.1f MB, on-the-fly %.1f MB, level 0 of the volume %.1f MB"
          % (peak[False] / 1e6, peak[True] / 1e6, vol0 / 1e6))
    assert states[True].corr0 is None and states[True].levels is None and states[False].corr0 is not None
    assert len(states[True].fpyr) == 3 and states[True].fpyr[0].dtype == torch.float32
    assert peak[False] - peak[True] >= 0.9 * vol0, peak


# ---------------------------------------------------------------------------------------------------------------------
# 6. graph
# ---------------------------------------------------------------------------------------------------------------------
def _finetune(ops, dev, synth, alt, precision="bf16"):
    import argparse
    net_mod = importlib.import_module("zero-tig_amd.network")
    net = net_mod.Finetunemodel(argparse.Namespace(dataset="RLV", of_scale=1, alternate_corr=alt), ops=ops, precision=precision)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(1).items()})
    net = net.to(dev)
    net.eval()
    return net


@pytest.mark.gpu
def test_inferstep_alternate_corr_replay_equals_eager(hip_ops, synth):
    """four 128 x 128 frames, of_scale 1: the replayed graph of the on-the-fly plan gives the bits of its eager launches, and the plan
    inside is the on-the-fly one (the flag reaches it through Finetunemodel's args)"""
    ops, dev = hip_ops
    infer = importlib.import_module("zero-tig_amd.infer")
    host = frames(synth, 4, 128, 128)
    res = []
    for use_graph in (False, True):
        net = _finetune(ops, dev, synth, True)
        step = infer.InferStep(net, use_graph=use_graph)
        n0 = {k: ops.lib.calls.get(k, 0) for k in ("zt_corr_lookup", "zt_corr_lookup_step", "zt_corr_alt_lookup_step", "zt_fmap_pyramid")}
        outs = []
        for t, x in enumerate(host):
            o = step(x.pin_memory() if use_graph else x.to(dev), is_new_seq=(t == 0))
            outs.append([v.clone() for v in o] + [v.clone() for v in step.u8])
        n = {k: ops.lib.calls.get(k, 0) - v for k, v in n0.items()}
        assert net._plan()[1].alternate_corr is True
        assert n["zt_corr_lookup"] == 0 and n["zt_corr_lookup_step"] == 0 and n["zt_corr_alt_lookup_step"] > 0 and n["zt_fmap_pyramid"] > 0, n
        assert (step.graph is not None) == use_graph
        res.append(outs)
    for t, (a, b) in enumerate(zip(*res)):
        for k, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (t, k, float((u.float() - v.float()).abs().max()))
    assert _finetune(ops, dev, synth, False)._plan()[1].alternate_corr is False


# ---------------------------------------------------------------------------------------------------------------------
# 7. the scripts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scripts_alternate_corr(tmp_path, synth):
    """predict.py --alternate_corr 1 and evals.py --tc 1 --tc_alternate_corr 1 on a four-frame 128 x 128 clip; the differences from
    the flag-0 runs are printed, not asserted (test 4 is the numeric gate)"""
    from test_evals_y4m import _frames_of, _payloads, _run, _weights, _write, _y4m
    head = _y4m().Header(128, 128, "25:1", "p", None, "420mpeg2", "LIMITED")
    fmt = head.format("bt709")
    clip = [(t, 2) for t in range(4)]
    src = _write(tmp_path / "low.y4m", head, _payloads(synth, fmt, clip, False))
    ref = _write(tmp_path / "gt.y4m", head, _payloads(synth, fmt, clip, True))
    common = ("--model_pretrain", _weights(tmp_path, synth), "--graph", "1", "--precision", "bf16", "--of_scale", "1", "--y4m_in", src)
    streams, temporal = {}, {}
    for alt in (1, 0):
        r = _run("predict.py", *common, "--save", tmp_path / ("pred%d" % alt), "--alternate_corr", alt)
        said = [line for line in r.stdout.split("\n") if "RAFT correlation:" in line]
        assert len(said) == 1 and ("on-the-fly" in said[0]) == bool(alt) and "16 x 16" in said[0] and "MB" in said[0], r.stdout[-2000:]
        streams[alt] = {}
        for kind in ("enhance", "denoise"):
            hd, fr = _frames_of(tmp_path / ("pred%d" % alt) / ("low_%s.y4m" % kind))
            assert (hd.W, hd.H, hd.ctag) == (head.W, head.H, head.ctag) and len(fr) == 4
            assert all(f.shape == fr[0].shape and f.dtype == fr[0].dtype for f in fr)
            streams[alt][kind] = fr
        r = _run("evals.py", *common, "--y4m_gt", ref, "--save", tmp_path / ("ev%d" % alt), "--tc", "1", "--tc_alternate_corr", alt)
        said = [line for line in r.stdout.split("\n") if "RAFT correlation:" in line]
        assert sum("on-the-fly" in line for line in said) == alt and len(said) == 2, said      # the model's plan and the metric's own
        temporal[alt] = json.load(open(str(tmp_path / ("ev%d" % alt) / "Metrics.json")))["temporal"]
    keys = {"scale", "size", "pairs", "raft", "valid_share", "E_warp", "E_static", "MABD", "E_warp_gt", "E_static_gt", "MABD_gt", "MABD_mse"}
    assert set(temporal[1]) == keys == set(temporal[0]) and temporal[1]["pairs"] == 3
    for kind in ("enhance", "denoise"):
        d = max(int(np.abs(x.astype(np.int64) - y.astype(np.int64)).max()) for x, y in zip(streams[1][kind], streams[0][kind]))
        print("CORRALT scripts: %s stream, largest sample difference between --alternate_corr 1 and 0: %d" % (kind, d))
    print("CORRALT scripts: temporal with --tc_alternate_corr 1 %r" % temporal[1])
    print("CORRALT scripts: temporal with --tc_alternate_corr 0 %r" % temporal[0])
