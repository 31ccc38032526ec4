"""LPIPS (VGG16) on the device: zt_conv3x3_wide_bf16, zt_lpips_prep, zt_maxpool2_nhwc, zt_lpips_layer, zero-tig_amd.lpips.LpipsVGG,
utils.lpips and evals.py --lpips_weights.

Neither lpips nor torchvision is installed and no weights file exists, so what is pinned is the DEFINITION (lpips 0.1, net='vgg',
eval mode), against `lpips_restated` below: plain torch on the CPU (F.conv2d / F.max_pool2d) in float64, written from the
definition, with seeded synthetic weights in the lpips state-dict key format (conv N(0, 2 / (9 Cin)), small biases, lin uniform
>= 0).  With such weights the five taps contribute about 63 / 29 / 6 / 1.4 / 0.9 % of the total, so every d_l is gated on its own.

Gates, all derived where the test runs (`_yardsticks`, once per session and size set):
* fp32 mode, every d_l and the total on its own: |d - d64| / d64 <= 20 x noise32, noise32 = the largest relative difference
  between the float32 and the float64 restatement over the yardstick cases and the six quantities.  20 x: the MFMA path sums K up
  to 4608 in another order and the normalisation divides small numbers at the deep taps.  The test asserts that this bound stays
  below a tenth of the bf16-operand difference measured the same way (the largest over the same cases and quantities when every
  conv's operands are rounded to bf16), so bf16 arithmetic cannot pass for fp32.  (A noise32 per quantity was tried and is not
  a yardstick: over two cases it is a sample of two -- d_4 of the 16 x 16 pair, a mean over four pixels, showed 2e-8 between the
  two restatements where d_5 showed 1.3e-6; the kernels' 6e-7 on d_4 is the same kind of noise.)
* bf16 mode: per quantity, |d - d64| / d64 <= 3 x (largest relative difference of that quantity between the bf16-operand float64
  restatement and the float64 restatement over the yardstick cases); 3 x because the device also stores the taps in bf16.
* yardstick cases: the lowlight and the random pair at every size of the backend's list below 1080p (the float64 restatement
  of one 1080p pair takes the better part of a minute; three variants of it would triple that for no new information).
* the wide conv alone: test_conv_bf16's form, max(|got - ref| - |ref| 2^-8) < 2e-3 against F.conv2d on bf16-rounded operands.
* prep / pool: bit for bit against torch.  zt_lpips_layer: 1e-5 relative against the float64 formula (fp32 per pixel: a few ulp
  per term, 2^-24 = 6e-8; the sum is fp64), an all-zero pixel included.

Host emulator cost of this file (`pytest tests/test_lpips.py -q -m "not gpu"`, 23 cases): 3.6 minutes on the 16-core build machine;
one 16 x 16 feature pass costs about 20 s there in fp32 mode (the exact fp32 conv kernel, fibre by fibre) and 7 s in bf16 mode."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ----------------------------------------------------------------------------------------------------------- the definition
VGG_CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
             (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)]      # features index, Cin, Cout
VGG_POOLS = (4, 9, 16, 23)                    # features indices of the MaxPool2d(2, 2) layers
VGG_TAPS = (3, 8, 15, 22, 29)                 # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
SLICE_OF = lambda idx: 1 + sum(idx > t for t in VGG_TAPS)        # lpips' vgg16 wrapper: slice1 = features[0:4], slice2 = [4:9], ...
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def synthetic_state_dict(seed=0, fmt="lpips"):
    g = torch.Generator().manual_seed(1234 + seed)
    sd = {}
    for idx, cin, cout in VGG_CONVS:
        stem = ("net.slice%d.%d." % (SLICE_OF(idx), idx)) if fmt == "lpips" else ("features.%d." % idx)
        sd[stem + "weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[stem + "bias"] = torch.randn(cout, generator=g) * 0.05
    for k, c in enumerate((64, 128, 256, 512, 512)):
        w = torch.rand(1, c, 1, 1, generator=g) / c
        sd["lin%d.model.1.weight" % k] = w
        if fmt == "lpips":
            sd["lins.%d.model.1.weight" % k] = w
    if fmt == "lpips":
        sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
        sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    return sd


def _bf(t):
    return t.to(torch.float32).bfloat16().to(t.dtype)


def taps_restated(img, sd, dtype, bf16_operands=False):
    x = (torch.as_tensor(img).to(dtype) - 0.5) * 2
    x = (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    convs = {idx: (cin, cout) for idx, cin, cout in VGG_CONVS}
    taps = []
    for idx in range(30):
        if idx in convs:
            s = "net.slice%d.%d." % (SLICE_OF(idx), idx)
            w, b = sd[s + "weight"].to(dtype), sd[s + "bias"].to(dtype)
            x = F.conv2d(_bf(x) if bf16_operands else x, _bf(w) if bf16_operands else w, b, padding=1)
        elif idx in VGG_POOLS:
            x = F.max_pool2d(x, 2, 2)
        else:
            x = F.relu(x)
        if idx in VGG_TAPS:
            taps.append(x)
    return taps


def distance_restated(ta, tb, sd):
    d = []
    for k, (fa, fb) in enumerate(zip(ta, tb)):
        na = fa / (torch.sqrt((fa ** 2).sum(1, keepdim=True)) + 1e-10)
        nb = fb / (torch.sqrt((fb ** 2).sum(1, keepdim=True)) + 1e-10)
        w = sd["lin%d.model.1.weight" % k].to(fa.dtype)
        d.append(float(((na - nb) ** 2 * w).sum(1, keepdim=True).mean(dim=(2, 3)).double()))
    return sum(d), d


def lpips_restated(a, b, sd, dtype=torch.float64, bf16_operands=False):
    with torch.no_grad():
        return distance_restated(taps_restated(a, sd, dtype, bf16_operands), taps_restated(b, sd, dtype, bf16_operands), sd)


# ----------------------------------------------------------------------------------------------------------- cases
def _pair(kind, synth, H, W):
    rng = np.random.default_rng(4000 + H * 7 + W)
    if kind == "lowlight":
        a = np.clip(synth.lowlight_frame(0, H, W) * np.float32(3), np.float32(1e-4), np.float32(1)).astype(np.float32)
        b = np.asarray(synth.clean_frame(0, H, W), dtype=np.float32).reshape(1, 3, H, W)
    elif kind == "random":
        a, b = rng.random((1, 3, H, W), dtype=np.float32), rng.random((1, 3, H, W), dtype=np.float32)
    else:
        a = rng.random((1, 3, H, W), dtype=np.float32)
        b = a.copy()
    return a, b


SIZES = {"emu": [(16, 16)], "hip": [(16, 16), (67, 93), (270, 480)]}
_CACHE = {}


def _ref64(kind, synth, H, W):
    key = ("ref", kind, H, W)
    if key not in _CACHE:
        a, b = _pair(kind, synth, H, W)
        _CACHE[key] = lpips_restated(a, b, synthetic_state_dict())
    return _CACHE[key]


def _yardsticks(name, synth):
    """-> (noise32, bf16 yardstick), each per quantity [d_1 .. d_5, total]: largest relative difference to the float64 restatement"""
    key = ("yard", name)
    if key not in _CACHE:
        sd = synthetic_state_dict()
        noise32, bfy = [0.0] * 6, [0.0] * 6
        for (H, W) in SIZES[name]:
            for kind in ("lowlight", "random"):
                a, b = _pair(kind, synth, H, W)
                t64, d64 = _ref64(kind, synth, H, W)
                t32, d32 = lpips_restated(a, b, sd, torch.float32)
                tbf, dbf = lpips_restated(a, b, sd, torch.float64, bf16_operands=True)
                q64, q32, qbf = d64 + [t64], d32 + [t32], dbf + [tbf]
                r32 = [abs(x - y) / y for x, y in zip(q32, q64)]
                rbf = [abs(x - y) / y for x, y in zip(qbf, q64)]
                print("yardstick %s %dx%d: fp32 %s bf16-operands %s" % (kind, H, W, ["%.2e" % v for v in r32], ["%.2e" % v for v in rbf]))
                noise32 = [max(u, v) for u, v in zip(noise32, r32)]
                bfy = [max(u, v) for u, v in zip(bfy, rbf)]
        _CACHE[key] = (noise32, bfy)
    return _CACHE[key]


def _model(ops, dev, precision, sd=None):
    mod = importlib.import_module("zero-tig_amd.lpips")
    return mod.LpipsVGG(ops, synthetic_state_dict() if sd is None else sd, dev, precision)


def _e2e_cases():
    out = []
    for kind in ("lowlight", "random"):
        out.append(pytest.param("emu", (16, 16), kind, id="emu-16x16-" + kind))
        for (h, w) in SIZES["hip"]:
            out.append(pytest.param("hip", (h, w), kind, id="hip-%dx%d-%s" % (h, w, kind), marks=pytest.mark.gpu))
    out.append(pytest.param("hip", (1080, 1920), "lowlight", id="hip-1080x1920-lowlight", marks=pytest.mark.gpu))
    return out


def _check(prec, name, synth, ours_total, ours_d, size, kind):
    H, W = size
    t64, d64 = _ref64(kind, synth, H, W)
    noise32, bfy = _yardsticks(name, synth)
    got, ref = ours_d + [ours_total], d64 + [t64]
    rel = [abs(x - y) / y for x, y in zip(got, ref)]
    if prec == "fp32":
        bound = [20.0 * max(noise32)] * 6
        print("lpips fp32 %s %dx%d: rel %s bound %.3g (fp32 restatement %s, bf16-operand restatement %s)" %
              (kind, H, W, ["%.2e" % v for v in rel], bound[0], ["%.2e" % v for v in noise32], ["%.2e" % v for v in bfy]))
        assert bound[0] < max(bfy) / 10.0, (bound[0], bfy)
    else:
        bound = [3.0 * v for v in bfy]
        print("lpips bf16 %s %dx%d: rel %s bound %s" % (kind, H, W, ["%.2e" % v for v in rel], ["%.2e" % v for v in bound]))
    for k, (r, bnd) in enumerate(zip(rel, bound)):
        assert r <= bnd, ("d_%d" % (k + 1) if k < 5 else "total", got[k], ref[k], r, bnd)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("backend,size,kind", _e2e_cases(), indirect=["backend"])
def test_lpips_parity(backend, synth, size, kind, precision):
    ops, dev, name = backend
    a, b = _pair(kind, synth, *size)
    m = _model(ops, dev, precision)
    fa, fb = m.features(torch.from_numpy(a).to(dev)), m.features(torch.from_numpy(b).to(dev))
    total, d = m.distance(fa, fb)
    assert len(d) == 5 and all(math.isfinite(v) and v >= 0 for v in d)
    _check(precision, name, synth, total, d, size, kind)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_lpips_properties(backend, synth, precision):
    """LPIPS(b, b) == 0 exactly from two separate feature passes; same input, same bits; cached ground-truth features give the
    bits of a fresh pass; a torchvision-named weights dict resolves to the same device weights.  (Three feature passes only: one
    costs 7 - 20 s in the host emulator.)"""
    ops, dev, name = backend
    a, b = _pair("random", synth, 16, 16)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    m = _model(ops, dev, precision)
    fa, fb, fb2 = m.features(ta), m.features(tb), m.features(tb.clone())
    assert all(torch.equal(u, v) for u, v in zip(fb, fb2))
    assert m.distance(fb, fb2) == (0.0, [0.0] * 5)
    first = m.distance(fa, fb)
    assert first[0] > 0.0 and m.distance(fa, fb2) == first and m.distance(fa, fb) == first
    m2 = _model(ops, dev, precision, synthetic_state_dict(fmt="torchvision"))      # features.<idx>.* + lin<k>
    assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(m.layers, m2.layers))
    assert all(torch.equal(u, v) for u, v in zip(m.lin, m2.lin))
    if name == "hip":
        assert m(ta, tb) == first[0] and m(tb, tb.clone()) == 0.0


def test_lpips_weights_errors(backend):
    ops, dev, _ = backend
    mod = importlib.import_module("zero-tig_amd.lpips")
    sd = synthetic_state_dict()
    missing = {k: v for k, v in sd.items() if ".17." not in k}
    with pytest.raises(ValueError, match=r"features\[17\].*missing.*keys found:.*net\.slice1\.0\.weight"):
        mod.LpipsVGG(ops, missing, dev)
    bad = dict(sd)
    bad["net.slice3.12.weight"] = torch.zeros(256, 128, 3, 3)
    with pytest.raises(ValueError, match=r"features\[12\].*shape"):
        mod.LpipsVGG(ops, bad, dev)
    nolin = {k: v for k, v in sd.items() if "lin3." not in k and "lins.3." not in k}
    with pytest.raises(ValueError, match="lin3 weight is missing"):
        mod.LpipsVGG(ops, nolin, dev)
    with pytest.raises(ValueError, match="precision"):
        mod.LpipsVGG(ops, sd, dev, "fp16")


# ----------------------------------------------------------------------------------------------------------- the wide conv
def _wide_cases():
    small = [(64, 128, 1, 9, 21), (128, 128, 2, 7, 19), (64, 128, 1, 2, 3), (256, 512, 1, 5, 6)]
    large = [(128, 256, 1, 13, 37), (256, 256, 2, 11, 18), (512, 512, 1, 9, 17), (512, 512, 2, 67, 120), (128, 128, 1, 135, 240)]
    out = [pytest.param("emu", c, id="emu-c%d-%d_n%d_%dx%d" % c) for c in small]
    out += [pytest.param("hip", c, id="hip-c%d-%d_n%d_%dx%d" % c, marks=pytest.mark.gpu) for c in small + large]
    return out


@pytest.mark.parametrize("backend,case", _wide_cases(), indirect=["backend"])
def test_conv3x3_wide_bf16(backend, case):
    """Every (Cin, Cout) VGG sends to the kernel, N in {1, 2}, ragged maps (not multiples of the 8 x 16 tile, odd, smaller than a
    tile), input and output pitches wider than the channel counts with NaN in the padding lanes."""
    CV = importlib.import_module("zero-tig_amd.ops").CV
    ops, dev, _ = backend
    Cin, Cout, N, H, W = case
    g = torch.Generator().manual_seed(Cin * 17 + Cout + H)
    x = torch.randn(N, Cin, H, W, generator=g).bfloat16().float()
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = torch.relu(F.conv2d(x, w.bfloat16().float(), b, padding=1))
    xd = torch.full((N, H, W, Cin + 8), float("nan")).bfloat16()
    xd[..., :Cin] = x.permute(0, 2, 3, 1).bfloat16()
    out = torch.full((N, H, W, Cout + 16), float("nan")).bfloat16().to(dev)
    wd = ops.repack_weight_bf16(w.to(dev))
    ops.conv3x3_wide_bf16(CV(xd.to(dev), 0, Cin), wd, b.to(dev), Cout, relu=True, out=CV(out, 8, Cout))
    got = out.float().cpu()[..., 8:8 + Cout].permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    err = float(((got - ref).abs() - ref.abs() * 2 ** -8).max())
    print("wide conv %s: err %.3g" % (case, err))
    assert err < 2e-3
    o = out.float().cpu()
    assert torch.isnan(o[..., :8]).all() and torch.isnan(o[..., 8 + Cout:]).all()      # nothing written outside the channel view
    nb = ops.conv3x3_wide_bf16(CV(xd.to(dev), 0, Cin), wd, None, Cout, relu=False)      # no bias, no ReLU, dense output
    refn = F.conv2d(x, w.bfloat16().float(), None, padding=1)
    assert float(((nb.float().cpu().permute(0, 3, 1, 2) - refn).abs() - refn.abs() * 2 ** -8).max()) < 2e-3


def test_conv3x3_wide_refuses_other_shapes(backend):
    CV = importlib.import_module("zero-tig_amd.ops").CV
    ops, dev, _ = backend
    for cin, cout in ((48, 128), (64, 64), (64, 192)):
        x = torch.zeros((1, 4, 4, cin), dtype=torch.bfloat16, device=dev)
        w = torch.zeros((9, cout, cin), dtype=torch.bfloat16, device=dev)
        with pytest.raises(RuntimeError, match="1001"):
            ops.conv3x3_wide_bf16(CV(x), w, None, cout)


# ----------------------------------------------------------------------------------------------------------- prep / pool / layer
@pytest.mark.parametrize("size", [(5, 7), (16, 16), (37, 54)])
def test_lpips_prep_bit_exact(backend, size):
    ops, dev, _ = backend
    H, W = size
    img = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(H))
    ref = ((img - 0.5) * 2 - torch.tensor(SHIFT).view(1, 3, 1, 1)) / torch.tensor(SCALE).view(1, 3, 1, 1)
    ref8 = torch.zeros(1, H, W, 8)
    ref8[..., :3] = ref.permute(0, 2, 3, 1)
    got = ops.lpips_prep(img.to(dev)).cpu()
    assert torch.equal(got.view(torch.int32), ref8.view(torch.int32))
    gotb = ops.lpips_prep(img.to(dev), torch.bfloat16).cpu()
    assert torch.equal(gotb.view(torch.int16), ref8.bfloat16().view(torch.int16))


@pytest.mark.parametrize("size", [(2, 2), (7, 9), (8, 6), (13, 16)])
def test_maxpool2_bit_exact(backend, size):
    CV = importlib.import_module("zero-tig_amd.ops").CV
    ops, dev, _ = backend
    H, W = size
    g = torch.Generator().manual_seed(H * 31 + W)
    for dtype, C, ld in ((torch.float32, 12, 16), (torch.bfloat16, 24, 32), (torch.bfloat16, 64, 64)):
        x = torch.randn(2, C, H, W, generator=g).to(dtype)
        ref = F.max_pool2d(x.float(), 2, 2).to(dtype).permute(0, 2, 3, 1).contiguous()
        xd = torch.full((2, H, W, ld), float("nan")).to(dtype)
        xd[..., :C] = x.permute(0, 2, 3, 1)
        got = ops.maxpool2(CV(xd.to(dev), 0, C)).cpu()
        assert got.shape == ref.shape and torch.equal(got.float(), ref.float())


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_lpips_layer(backend, C, dtype):
    ops, dev, _ = backend
    g = torch.Generator().manual_seed(C)
    H, W = 5, 13                                                       # 65 pixels: ragged against every pixels-per-workgroup count
    fa = torch.relu(torch.randn(1, H, W, C, generator=g)).to(dtype)
    fb = torch.relu(torch.randn(1, H, W, C, generator=g)).to(dtype)
    fa[0, 2, 3] = 0                                                    # an all-zero pixel in one map, and in both
    fa[0, 4, 12] = 0
    fb[0, 4, 12] = 0
    w = torch.rand(C, generator=g) / C
    a64, b64 = fa.double(), fb.double()
    na = a64 / (torch.sqrt((a64 ** 2).sum(-1, keepdim=True)) + 1e-10)
    nb = b64 / (torch.sqrt((b64 ** 2).sum(-1, keepdim=True)) + 1e-10)
    ref = float((((na - nb) ** 2) * w.double()).sum(-1).mean())
    out = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    ops.lpips_layer(fa.to(dev), fb.to(dev), w.to(dev), out[1:2])
    got = float(out[1])
    print("lpips layer C=%d %s: got %.17g ref %.17g rel %.3g" % (C, dtype, got, ref, abs(got - ref) / ref))
    assert math.isfinite(got) and float(out[0]) == -1.0 and abs(got - ref) <= 1e-5 * ref
    ops.lpips_layer(fa.to(dev), fa.clone().to(dev), w.to(dev), out[0:1])
    assert float(out[0]) == 0.0


# ----------------------------------------------------------------------------------------------------------- evals.py
@pytest.mark.gpu
def test_evals_script_reports_lpips(tmp_path, synth):
    """evals.py --lpips_weights on a four-frame clip: Total_LPIPS / Total_LPIPS_HM are finite floats >= 0 and the log carries the
    per-frame values; PSNR / SSIM fields are bit-identical to a run without the flag, whose LPIPS fields stay null."""
    from PIL import Image
    data = tmp_path / "data" / "RLV"
    for kind, sub, fn in (("input", "low_light_10", synth.lowlight_frame), ("gt", "normal_light_10", synth.clean_frame)):
        d = data / kind / "S01" / sub
        d.mkdir(parents=True)
        for t in range(4):
            a = np.asarray(fn(t, 270, 480), dtype=np.float32)
            im = (np.transpose(a[0] if a.ndim == 4 else a, (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
            Image.fromarray(im).save(str(d / ("%05d.png" % (t + 1))))
    (data / "train_list.txt").write_text("S01\n")
    (data / "test_list.txt").write_text("S01\n")
    weights = tmp_path / "weights.pt"
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, str(weights))
    lw = tmp_path / "lpips_vgg.pt"
    torch.save(synthetic_state_dict(), str(lw))
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run_evals(save, *extra):
        r = subprocess.run([sys.executable, "evals.py", "--dataset", "RLV", "--lowlight_images_path", str(data), "--model_pretrain",
                            str(weights), "--save", str(save)] + list(extra), cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        return json.load(open(save / "Metrics.json")), r.stdout

    m0, out0 = run_evals(tmp_path / "ev0")
    assert m0["Total_LPIPS"] is None and m0["Total_LPIPS_HM"] is None and "LPIPS" not in out0
    for prec in ("fp32", "bf16"):
        m, out = run_evals(tmp_path / ("ev_" + prec), "--lpips_weights", str(lw), "--lpips_precision", prec)
        print(prec, m)
        for k in ("Total_LPIPS", "Total_LPIPS_HM"):
            assert isinstance(m[k], float) and math.isfinite(m[k]) and m[k] >= 0.0, (k, m)
        assert "LPIPS: " in out and "LPIPS_HM: " in out and "Total LPIPS: " in out
        for k in ("Total_PSNR", "Total_SSIM", "Total_PSNR_HM", "Total_SSIM_HM", "images"):
            assert m[k] == m0[k], (k, m[k], m0[k])
    mh, _ = run_evals(tmp_path / "ev_nohm", "--lpips_weights", str(lw), "--hist_match", "0")
    assert isinstance(mh["Total_LPIPS"], float) and mh["Total_LPIPS_HM"] is None
