"""csrc/zt_flowviz.hip -- `Ops.flow_radmax`, `flow_to_rgb`, `flow_pack`, `tc_viz` -- and zero-tig_amd/flowio.py, on the host
emulator and, under -m gpu, on the MI355X.

1. Against a numpy float32 restatement of the definitions, BIT FOR BIT: every operation of the kernels is IEEE fp32 with one rounding
   (no fused multiply-add, no library transcendental; sqrt and / are correctly rounded on both sides), the maximum does not depend on
   the order it is taken in, and nothing else is reduced.  The four panels of `tc_viz` are built on `restate()` of test_temporal.py,
   the restatement `zt_warp_error_f32` is held to.
2. Against what the reference's `utils/flow_viz.py` and `utils/frame_utils.py` produced for the same flows, recorded in
   tests/golden/g13_flowviz.npz by tools/make_flowviz_golden.py (which asserts every gate below on the restatement before it writes
   the file).  The reference takes its angle from `np.arctan2` and divides by pi, the kernels from a polynomial whose largest error is
   2.7e-7 rad, in float32: a sample can land on the other side of a floor.  Gate: no sample differs by more than one
   level, and at most 20 of the 196 608 samples of a 256 x 256 picture differ (1e-4; the restatement differed in 0 to 3 on 16 such
   fixtures, the reference in float32 from itself in float64 in 1 to 5 per 1.5 M).  The 40 x 72 flow, the axis directions, both
   signed zeros and the zero flow: equal.  The compass goes through the same two paths as the other flows (scaled by its own
   largest radius, and by 6): drawn unscaled, a radius of exactly 1 on an exact wheel entry sits on the edge of a floor --
   1 - 1 * (1 - 43/255) is 42.99999 in fp32 and 43 in the reference's float64 colours -- which no fp32 restatement of
   `1 - rad * (1 - col)` can meet.  Measured on the restatement (the kernels equal it): 1, 0, 0 and 0 samples differ on the four
   256 x 256 pictures, none on the compass.  The noise flow is used as the generator draws it: rounded to 1/64 pixel, as the
   smooth one is to keep a sine's last bit out of it, its scaled components fall on a lattice where many products sit on a
   floor's edge, and 10 to 17 samples of the picture over 6 differed on six seeds, against 0 or 1 unrounded.

The rule for values that cannot be drawn: a pixel is black when un^2 + vn^2 is not finite -- a NaN or infinite component, or one
whose square overflows (1e30) -- and `flow_radmax` passes over the pixels whose u^2 + v^2 is not finite, so the scale itself is
always finite."""
import os
import zlib

import numpy as np
import pytest
import torch

from test_temporal import KINDS, SIZES, _case, _place, _smooth, restate

F = np.float32
PI, PI_2, PI_4 = F(3.14159274), F(1.57079637), F(0.785398185)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_flowviz.npz")


# --------------------------------------------------------------------------------------------------------- the restatement
def wheel_levels():
    """the 55 x 3 wheel from the six segment lengths of Baker et al. 2007"""
    seg, full, ramp = (15, 6, 4, 11, 13, 6), (0, 1, 1, 2, 2, 0), (1, 0, 2, 1, 0, 2)
    rows = []
    for s in range(6):
        for i in range(seg[s]):
            row = [0, 0, 0]
            row[full[s]] = 255
            row[ramp[s]] = 255 * i // seg[s] if s % 2 == 0 else 255 - 255 * i // seg[s]
            rows.append(row)
    return np.array(rows, np.uint8)


def np_angle(y, x):
    """atan2(y, x) by the kernel's sequence of float32 operations"""
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.where(ax > ay, ax, ay), np.where(ax > ay, ay, ax)
    with np.errstate(all="ignore"):
        t = np.where(mx == F(0), F(0), mn / mx)
        big = t > F(0.41421357)
        t = np.where(big, (t - F(1)) / (t + F(1)), t)
    base = np.where(big, PI_4, F(0))
    z = t * t
    p = F(8.05374449538e-2) * z - F(1.38776856032e-1)
    p = p * z + F(1.99777106478e-1)
    p = p * z - F(3.33329491539e-1)
    p = p * z
    p = p * t + t
    a = base + p
    a = np.where(ay > ax, PI_2 - a, a)
    a = np.where(np.signbit(x), PI - a, a)
    a = np.copysign(a, y)
    assert a.dtype == F
    return a


def np_flow_levels(u, v, radius, bgr=False):
    """u, v float32 [H, W], radius a float32 -> uint8 [H, W, 3]"""
    assert u.dtype == F and v.dtype == F
    wheel = wheel_levels().astype(F) / F(255)
    with np.errstate(all="ignore"):
        den = F(radius) + F(1e-5)
        un, vn = u / den, v / den
        r2 = un * un + vn * vn
        ok = r2 < F(np.inf)
        un, vn, r2 = np.where(ok, un, F(0)), np.where(ok, vn, F(0)), np.where(ok, r2, F(0))
        rad = np.sqrt(r2)
        fk = (np_angle(-vn, -un) / PI + F(1)) * F(27)
        fl = np.floor(fk)
        k0 = np.clip(fl.astype(np.int64), 0, 54)
        k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
        f = fk - fl
        out = np.zeros(u.shape + (3,), np.uint8)
        for c in range(3):
            col = (F(1) - f) * wheel[k0, c] + f * wheel[k1, c]
            col = np.where(rad <= F(1), F(1) - rad * (F(1) - col), col * F(0.75))
            assert col.dtype == F
            level = np.clip(np.floor(F(255) * col).astype(np.int64), 0, 255)
            out[..., 2 - c if bgr else c] = np.where(ok, level, 0)
    return out


def np_radmax(flows, win):
    m = F(0)
    with np.errstate(all="ignore"):
        for fl in flows:
            u, v = fl[0][win], fl[1][win]
            r2 = u * u + v * v
            r = np.sqrt(r2[r2 < F(np.inf)])
            m = max(m, r.max()) if r.size else m
    return F(m)


def np_tc_viz(cur, prev, fb, ff, oy, ox, radius, gain):
    """-> float32 [3, 2H, 2W], from `restate()` of test_temporal.py"""
    _, H, W = cur.shape
    out = np.zeros((3, 2 * H, 2 * W), F)
    if prev is None:
        out[:, :H] = 1
        out[:, H:, :W] = cur
        return out
    win = (slice(oy, oy + H), slice(ox, ox + W))
    _, _, valid, e, inside = restate(cur, prev, fb, ff, oy, ox)
    for flow, x0 in ((fb, 0), (ff, W)):
        lv = np_flow_levels(flow[0][win], flow[1][win], radius)
        out[:, :H, x0:x0 + W] = (lv.astype(F) / F(255)).transpose(2, 0, 1)
    flag = np.where(inside, np.array([0, 1, 1], F)[:, None, None], np.array([1, 0, 1], F)[:, None, None])
    out[:, H:, :W] = np.where(valid, cur, flag)
    with np.errstate(all="ignore"):
        g = np.minimum(F(1), np.sqrt(e / F(3)) * F(gain))
    out[:, H:, W:] = np.where(valid, g, F(0))
    return out


# --------------------------------------------------------------------------------------------------------- the cases
GAIN = 4.0
_VIZ = {}


def _viz_case(kind, size):
    """the case of test_temporal.py with its images mapped into [0.05, 0.95] (no pixel equals a flag colour), and a radius: the
    joint largest radius of the two flows; the planted kind takes the radius of the smooth kind, so that the two can be compared"""
    key = (kind, size)
    if key not in _VIZ:
        cur, prev, fb, ff, oy, ox, _ = _case(kind, size)
        cur, prev = (F(0.05) + F(0.9) * a for a in (cur, prev))
        H, W = size[:2]
        win = (slice(oy, oy + H), slice(ox, ox + W))
        src = _case("smooth", size) if kind == "planted" else (cur, prev, fb, ff)
        radius = np_radmax((src[2], src[3]), win)
        for a in (cur, prev):
            a.setflags(write=False)
        _VIZ[key] = (cur, prev, fb, ff, oy, ox, win, radius)
    return _VIZ[key]


def _out(shape, dtype, dev, offset=0):
    """an output view `offset` elements behind a 16-byte aligned address, and a check that nothing around it was written"""
    n = int(np.prod(shape))
    buf = torch.full((n + offset + 16,), 77, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0

    def untouched():
        return bool((buf[:offset] == 77).all()) and bool((buf[offset + n:] == 77).all())
    return buf[offset:offset + n].view(shape), untouched


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _check_all(ops, dev, kind, size, offset):
    H, W, Hf, Wf = size
    cur, prev, fb, ff, oy, ox, win, radius = _viz_case(kind, size)
    tcur, tprev, tfb, tff = (_place(a, dev, offset) for a in (cur, prev, fb, ff))
    own = kind != "planted"                                  # the scale from the device, through flow_radmax
    # ---- radmax: one flow, two flows
    r1, r2 = ops.flow_radmax(tfb, h=H, w=W), ops.flow_radmax(tfb, tff, h=H, w=W)
    assert r1.dtype == torch.float32 and r1.device.type == dev.type
    ref1, ref2 = np_radmax((fb,), win), np_radmax((fb, ff), win)
    assert np.isfinite(ref2) and F(r1.item()).tobytes() == ref1.tobytes() and F(r2.item()).tobytes() == ref2.tobytes(), (r1, ref1, r2, ref2)
    assert _bytes(ops.flow_radmax(tfb, tff, h=H, w=W)) == _bytes(r2)
    if own:
        assert ref2 == radius
    # ---- the wheel: both outputs, both channel orders
    for bgr in (False, True):
        ref = np_flow_levels(fb[0][win], fb[1][win], ref1 if own else radius, bgr)
        rad = None if own else float(radius)
        u8, untouched = _out((H, W, 3), torch.uint8, dev, offset)
        ops.flow_to_rgb(tfb, H, W, radius=rad, u8=True, bgr=bgr, out=u8)
        assert np.array_equal(u8.cpu().numpy(), ref), (kind, size, bgr, int((u8.cpu().numpy() != ref).sum()))
        assert untouched()
        f32, untouched = _out((1, 3, H, W), torch.float32, dev, offset)
        ops.flow_to_rgb(tfb, H, W, radius=rad, bgr=bgr, out=f32)
        assert f32.cpu().numpy().tobytes() == (ref.astype(F) / F(255)).transpose(2, 0, 1).tobytes()
        assert untouched()
        assert _bytes(ops.flow_to_rgb(tfb, H, W, radius=rad, u8=True, bgr=bgr)) == ref.tobytes()
    # ---- the .flo payload
    pk, untouched = _out((H, W, 2), torch.float32, dev, offset)
    ops.flow_pack(tfb, H, W, out=pk)
    want = np.ascontiguousarray(np.stack([fb[0][win], fb[1][win]], axis=-1))
    assert pk.cpu().numpy().tobytes() == want.tobytes() and _bytes(ops.flow_pack(tfb, H, W)) == want.tobytes()
    assert untouched()
    # ---- the four panels
    ref = np_tc_viz(cur, prev, fb, ff, oy, ox, radius, GAIN)
    pic, untouched = _out((1, 3, 2 * H, 2 * W), torch.float32, dev, offset)
    ops.tc_viz(tcur, tprev, tfb, tff, r2 if own else float(radius), GAIN, out=pic)
    got = pic.cpu().numpy()[0]
    for name, (ys, xs) in {"backward flow": (slice(0, H), slice(0, W)), "forward flow": (slice(0, H), slice(W, 2 * W)),
                           "mask": (slice(H, 2 * H), slice(0, W)), "error": (slice(H, 2 * H), slice(W, 2 * W))}.items():
        assert got[:, ys, xs].tobytes() == ref[:, ys, xs].tobytes(), (kind, size, name, int((got[:, ys, xs] != ref[:, ys, xs]).sum()))
    assert untouched()
    assert _bytes(ops.tc_viz(tcur, tprev, tfb, tff, float(radius), GAIN)) == ref.tobytes()
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    # ---- the mask panel shows the pixels zt_warp_error_f32 counts
    n = int(ops.warp_error(tcur, tprev, tfb, tff)[0].item())
    bl = got[:, H:, :W]
    magenta = (bl[0] == 1) & (bl[1] == 0) & (bl[2] == 1)
    cyan = (bl[0] == 0) & (bl[1] == 1) & (bl[2] == 1)
    assert H * W - int(magenta.sum()) - int(cyan.sum()) == n, (kind, size, n, int(magenta.sum()), int(cyan.sum()))
    # ---- a frame without a partner
    ref0 = np_tc_viz(cur, None, None, None, 0, 0, None, GAIN)
    assert _bytes(ops.tc_viz(tcur, None, None, None, None, GAIN)) == ref0.tobytes()
    return got


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-in-%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_flowviz_parity(backend, kind, size):
    ops, dev, _ = backend
    _check_all(ops, dev, kind, size, 0)


@pytest.mark.parametrize("kind", ["smooth", "planted"])
def test_flowviz_unaligned_pointers(backend, kind):
    """136 x 200 and 16 x 64 in 24 x 72 take the 16-byte paths from aligned buffers; one float (one byte for the uint8 picture)
    further on the same values go value by value"""
    ops, dev, _ = backend
    for size in ((136, 200, 136, 200), (16, 64, 24, 72)):
        _check_all(ops, dev, kind, size, 1)


def test_flow_to_rgb_mixed_alignment(backend):
    """16 x 64 in 24 x 72: the flow, the uint8 picture and the planar picture are each either 16-byte aligned or one element off,
    in all eight combinations, both pictures written by one call: the wide and the narrow path of each are chosen on their own"""
    ops, dev, _ = backend
    H, W, Hf, Wf = size = (16, 64, 24, 72)
    _, _, fb, _, oy, ox, win, radius = _viz_case("smooth", size)
    ref = np_flow_levels(fb[0][win], fb[1][win], radius)
    rad = torch.full((1,), float(radius), dtype=torch.float32, device=dev)
    for bits in range(8):
        tfb = _place(fb, dev, bits & 1)
        u8, u8_untouched = _out((H, W, 3), torch.uint8, dev, bits >> 1 & 1)
        f32, f32_untouched = _out((1, 3, H, W), torch.float32, dev, bits >> 2 & 1)
        ops.lib.call("zt_flow_to_rgb", tfb, H, W, Hf, Wf, oy, ox, rad, u8, f32, 0, None if dev.type == "cpu" else ops._s(tfb))
        assert np.array_equal(u8.cpu().numpy(), ref), bits
        assert f32.cpu().numpy().tobytes() == (ref.astype(F) / F(255)).transpose(2, 0, 1).tobytes(), bits
        assert u8_untouched() and f32_untouched(), bits


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-in-%dx%d" % s)
def test_flowviz_planted_values(backend, size):
    """NaN, inf and +-1e30 in a flow: those pixels are black in its wheel panel, every value of the picture stays finite and in
    [0, 1], and no pixel that reads no planted value changes"""
    ops, dev, _ = backend
    H, W = size[:2]
    cur, prev, fb, ff, oy, ox, win, radius = _viz_case("planted", size)
    _, _, fb0, ff0, _, _, _, radius0 = _viz_case("smooth", size)
    assert radius == radius0
    pics = []
    for a, b in ((fb, ff), (fb0, ff0)):
        t = [_place(x, dev) for x in (cur, prev, a, b)]
        pics.append(ops.tc_viz(*t, float(radius), GAIN).cpu().numpy()[0])
    got, got0 = pics
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    own = np.zeros((H, W), bool)                             # pixels whose own backward flow was planted
    hit = np.zeros((H, W), bool)                             # planted samples of the forward flow
    for c in range(2):
        own |= ~(fb[c][win] == fb0[c][win])
        hit |= ~(ff[c][win] == ff0[c][win])
    assert own.any() and hit.any()
    assert (got[:, :H, :W][:, own] == 0).all() and (got[:, :H, W:][:, hit] == 0).all()
    assert (got[:, :H, :W][:, ~own] == got0[:, :H, :W][:, ~own]).all() and (got[:, :H, W:][:, ~hit] == got0[:, :H, W:][:, ~hit]).all()
    # readers of a planted forward flow: the four taps of every pixel, taken from the unplanted case
    inside0 = restate(cur, prev, fb0, ff0, oy, ox)[4]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        px = np.where(inside0, xs.astype(F) + fb0[0][win], F(0))
        py = np.where(inside0, ys.astype(F) + fb0[1][win], F(0))
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    rest = ~(own | hit[y0, x0] | hit[y0, x1] | hit[y1, x0] | hit[y1, x1])
    assert (got[:, H:][:, np.concatenate([rest, rest], axis=1)] == got0[:, H:][:, np.concatenate([rest, rest], axis=1)]).all()


def test_flowviz_argument_errors(backend):
    ops, dev, _ = backend
    img = torch.zeros(3 * 8 * 8, dtype=torch.float32, device=dev)
    flow = torch.zeros(2 * 16 * 16, dtype=torch.float32, device=dev)
    ws, r1 = torch.zeros(8, dtype=torch.float32, device=dev), torch.ones(1, dtype=torch.float32, device=dev)
    u8 = torch.zeros(8 * 8 * 3, dtype=torch.uint8, device=dev)
    f32 = torch.zeros(12 * 8 * 8, dtype=torch.float32, device=dev)
    geo = dict(H=8, W=8, Hf=16, Wf=16, oy=4, ox=4)

    def radmax(fa=flow, fb=None, w=ws, nblk=4, o=r1, **kw):
        g = dict(geo, **kw)
        ops.lib.call("zt_flow_radmax_f32", fa, fb, g["H"], g["W"], g["Hf"], g["Wf"], g["oy"], g["ox"], w, nblk, o, None)

    def to_rgb(fl=flow, r=r1, a=u8, b=f32, bgr=0, **kw):
        g = dict(geo, **kw)
        ops.lib.call("zt_flow_to_rgb", fl, g["H"], g["W"], g["Hf"], g["Wf"], g["oy"], g["ox"], r, a, b, bgr, None)

    def pack(fl=flow, o=f32, **kw):
        g = dict(geo, **kw)
        ops.lib.call("zt_flow_pack_hwc_f32", fl, g["H"], g["W"], g["Hf"], g["Wf"], g["oy"], g["ox"], o, None)

    def viz(c=img, p=img, a=flow, b=flow, r=r1, gain=4.0, o=f32, **kw):
        g = dict(geo, **kw)
        ops.lib.call("zt_tc_viz_f32", c, p, a, b, g["H"], g["W"], g["Hf"], g["Wf"], g["oy"], g["ox"], r, gain, o, None)
    for fn in (radmax, to_rgb, pack, viz):
        fn()                                                                     # the well-formed call
    assert r1.tolist() == [0.0]
    r1.fill_(1.0)
    viz(p=None, a=None, b=None, r=None)
    window = [{"Hf": 11}, {"Wf": 11}, {"oy": 9}, {"ox": 9}, {"oy": -1}, {"ox": -1}, {"H": 0}, {"W": 0}, {"H": -8}]
    bad = [(radmax, kw) for kw in window + [{"nblk": 0}, {"nblk": 4097}, {"fa": None}, {"w": None}, {"o": None}]]
    bad += [(to_rgb, kw) for kw in window + [{"fl": None}, {"r": None}, {"a": None, "b": None}, {"bgr": 2}]]
    bad += [(pack, kw) for kw in window + [{"fl": None}, {"o": None}]]
    bad += [(viz, kw) for kw in window + [{"c": None}, {"a": None}, {"b": None}, {"r": None}, {"o": None}, {"gain": -1.0},
                                          {"gain": float("nan")}, {"gain": float("inf")}]]
    for fn, kw in bad:
        with pytest.raises(RuntimeError, match="1001"):
            fn(**kw)
    with pytest.raises(AssertionError):                                          # the wrappers check the shapes
        ops.flow_pack(flow.view(1, 2, 16, 16), 17, 8)
    with pytest.raises(AssertionError):
        ops.tc_viz(img.view(1, 3, 8, 8), img.view(1, 3, 8, 8), flow[:72].view(1, 2, 6, 6), flow[:72].view(1, 2, 6, 6), 1.0, 4.0)


# --------------------------------------------------------------------------------------------------------- against the reference
COMPASS_RADII = (0.25, 1.0, 3.0)


def golden_inputs():
    """the flows whose pictures the golden file records, [H, W, 2] float32.  The 256 x 256 ones are made here and the file holds
    their CRC-32: the noise as the generator draws it, the smooth one rounded to 1/64 pixel so that the last bit of a sine cannot
    matter; the small ones are stored in the file."""
    rng = np.random.default_rng(13)
    noise = (4.0 * rng.standard_normal((256, 256, 2))).astype(F)
    smooth = (np.round(_smooth(np.random.default_rng(14), 256, 256, 6.0).astype(np.float64) * 64) / 64).astype(F).transpose(1, 2, 0)
    small = np.ascontiguousarray(_smooth(np.random.default_rng(0), 40, 72, 6.0).transpose(1, 2, 0))
    s = np.sqrt(0.5)
    rows = []
    for r in COMPASS_RADII:                                  # E, SE, S, SW, W, NW, N, NE: axis directions at the even places
        rows += [(r * a, r * b) for a, b in ((1, 0.0), (s, s), (0.0, 1), (-s, s), (-1, 0.0), (-s, -s), (0.0, -1), (s, -s))]
    rows += [(1, 0.0), (1, -0.0), (-1, 0.0), (-1, -0.0), (0.0, 0.0)]
    compass = np.array(rows, F).reshape(1, -1, 2)
    return {"noise": np.ascontiguousarray(noise), "smooth": np.ascontiguousarray(smooth), "small": small, "compass": compass}


COMPASS_AXES = [i for i in range(29) if i >= 24 or i % 2 == 0]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def gate(ours, ref, what, cap=20):
    d = np.abs(ours.astype(np.int64) - ref.astype(np.int64))
    print("%s: %d of %d samples differ, largest difference %d" % (what, int((d > 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1 and (d > 0).sum() <= cap, (what, int(d.max()), int((d > 0).sum()))


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLDEN))
    flows = golden_inputs()
    for name in ("noise", "smooth"):
        assert crc(flows[name]) == int(g["crc_" + name]), "the generator of the %r flow no longer makes the recorded flow" % name
    flows["small"], flows["compass"] = g["small_flow"], g["compass_flow"]
    return g, flows


def _dev_flow(flow_hw2, dev):
    return torch.from_numpy(np.ascontiguousarray(flow_hw2.transpose(2, 0, 1))[None]).to(dev)


def check_golden(render, g, flows):
    """`render(flow [H, W, 2], radius or None, bgr) -> uint8 [H, W, 3]` against every recorded picture"""
    den6 = F(6) + F(1e-5)
    for name in ("noise", "smooth"):
        gate(render(flows[name], None, False), g[name + "_image"], name + " flow_to_image")
        gate(render(flows[name], 6.0, False), g[name + "_colors6"], name + " flow_uv_to_colors / 6")
        un = flows[name] / den6
        share = float((np.sqrt(un[..., 0] ** 2 + un[..., 1] ** 2) > 1).mean())
        assert 0.2 <= share <= 0.5, (name, share)             # the out-of-range branch is reached
    assert np.array_equal(render(flows["small"], None, False), g["small_image"])
    assert np.array_equal(render(flows["small"], None, True), g["small_image_bgr"])
    assert np.array_equal(g["small_image_bgr"], g["small_image"][..., ::-1])
    # the compass, scaled by its own largest radius (3) and by 6: the axis directions, both signed zeros and the zero flow are equal
    for radius, key in ((None, "compass_image"), (6.0, "compass_colors6")):
        got, ref = render(flows["compass"], radius, False), g[key]
        assert np.array_equal(got[0, COMPASS_AXES], ref[0, COMPASS_AXES]), (key, got[0, COMPASS_AXES], ref[0, COMPASS_AXES])
        gate(got, ref, key, cap=3 * 12)
        # a rightward flow with v = +0 sits on wheel entry 0 (pure red: green and blue fade alike), with v = -0 on entry 54 (blue in
        # it), a leftward flow on entry 27 whatever the sign of its zero; zero flow is white
        assert ref[0, 24, 1] == ref[0, 24, 2] and ref[0, 25, 2] > ref[0, 25, 1] and tuple(ref[0, 24]) == tuple(ref[0, 8])
        assert tuple(ref[0, 26]) == tuple(ref[0, 27]) and tuple(ref[0, 28]) == (255, 255, 255)


def test_golden_restatement(gold):
    """the restatement itself meets the gates (what the tool asserted when it wrote the file)"""
    g, flows = gold

    def render(flow, radius, bgr):
        win = (slice(None), slice(None))
        r = np_radmax((flow.transpose(2, 0, 1),), win) if radius is None else radius
        return np_flow_levels(np.ascontiguousarray(flow[..., 0]), np.ascontiguousarray(flow[..., 1]), r, bgr)
    check_golden(render, g, flows)
    assert np.array_equal(wheel_levels(), g["wheel"])


def test_golden_kernels(backend, gold):
    ops, dev, _ = backend
    g, flows = gold

    def render(flow, radius, bgr):
        return ops.flow_to_rgb(_dev_flow(flow, dev), radius=radius, u8=True, bgr=bgr).cpu().numpy()
    check_golden(render, g, flows)
    assert np.array_equal(ops.flow_wheel().numpy(), g["wheel"])


@pytest.mark.gpu
def test_golden_dropins(gold):
    """utils/flow_viz.py: numpy in, numpy out, computed on the device"""
    from utils import flow_viz
    g, flows = gold

    def render(flow, radius, bgr):
        if radius is None:
            return flow_viz.flow_to_image(flow, convert_to_bgr=bgr)
        den = F(radius) + F(1e-5)
        return flow_viz.flow_uv_to_colors(flow[..., 0] / den, flow[..., 1] / den, convert_to_bgr=bgr)
    check_golden(render, g, flows)
    got = flow_viz.flow_to_image(flows["smooth"], clip_flow=2.0)
    assert got.dtype == np.uint8 and got.shape == (256, 256, 3)
    gate(got, g["smooth_image_clip2"], "smooth clip_flow=2.0")
    assert np.array_equal(flow_viz.make_colorwheel(), g["wheel"].astype(np.float64))


# --------------------------------------------------------------------------------------------------------- .flo files
def test_flo_writer_bytes(backend, gold, tmp_path):
    """`FloWriter` behind `flow_pack` of a 33 x 130 window in 40 x 136 writes the bytes the reference's writeFlow wrote"""
    import importlib
    flowio = importlib.import_module("zero-tig_amd.flowio")
    ops, dev, _ = backend
    g, _ = gold
    ref = g["flo_bytes"].tobytes()
    flow = np.frombuffer(ref, dtype="<f4", offset=12).reshape(33, 130, 2)
    padded = np.random.default_rng(5).uniform(-50, 50, (2, 40, 136)).astype(F)
    padded[:, 3:36, 3:133] = flow.transpose(2, 0, 1)
    writer = flowio.FloWriter(slots=2)
    paths = [str(tmp_path / ("%d.flo" % i)) for i in range(5)]      # more files than slots
    for p in paths:
        writer.submit(p, ops.flow_pack(_place(padded, dev), 33, 130))
    writer.close()
    assert writer.files == 5 and writer.bytes == 5 * len(ref)
    for p in paths:
        assert open(p, "rb").read() == ref
    back = flowio.read_flo(paths[0])
    assert back.dtype == np.float32 and back.shape == (33, 130, 2) and back.tobytes() == flow.tobytes()
    # the host-side pair, and the reference's names over it
    flowio.write_flo(str(tmp_path / "w.flo"), flow)
    assert open(str(tmp_path / "w.flo"), "rb").read() == ref
    from utils import frame_utils
    frame_utils.writeFlow(str(tmp_path / "a.flo"), flow)
    frame_utils.writeFlow(str(tmp_path / "b.flo"), flow[..., 0], flow[..., 1])
    assert open(str(tmp_path / "a.flo"), "rb").read() == ref and open(str(tmp_path / "b.flo"), "rb").read() == ref
    assert frame_utils.readFlow(str(tmp_path / "a.flo")).tobytes() == flow.tobytes()


def test_flo_errors(tmp_path):
    import importlib
    flowio = importlib.import_module("zero-tig_amd.flowio")
    good = tmp_path / "good.flo"
    flowio.write_flo(str(good), np.zeros((3, 5, 2), F))
    data = good.read_bytes()
    assert len(data) == 12 + 3 * 5 * 8 and data[:4] == b"PIEH"
    for name, blob in (("short.flo", data[:-4]), ("header.flo", data[:7]), ("tag.flo", b"HEIP" + data[4:]), ("long.flo", data + b"\0"),
                       ("size.flo", data[:4] + b"\0" * 8)):
        (tmp_path / name).write_bytes(blob)
        with pytest.raises(ValueError, match=name):
            flowio.read_flo(str(tmp_path / name))
    with pytest.raises(ValueError, match="bad.flo"):
        flowio.write_flo(str(tmp_path / "bad.flo"), np.zeros((3, 5), F))
    # an error of the writer thread surfaces on close()
    writer = flowio.FloWriter()
    writer.submit(str(tmp_path / "no" / "such" / "dir.flo"), np.zeros((3, 5, 2), F))
    with pytest.raises(OSError):
        writer.close()
