"""evals.py metrics on the device: SSIM (zt_ssim_u8_f32) and histogram matching (zt_match_histograms_f32).

skimage is not installed, so parity is against a restatement of its algorithms from the published definitions, written here with
numpy and scipy only: structural_similarity on uint8 input is five `uniform_filter(size=7)` passes in float64 with the sample
covariance (49/48) and a 3-pixel crop; match_histograms with channel_axis=None is `np.unique` + `np.interp` on the pooled values.

Gates and where they come from:
* SSIM: |ours - ssim_ref| <= 1e-9.  The integer-window-sum form and scipy's running-sum form, both in fp64, differ by 2.8e-17 at
  30x44 and 1.6e-15 at 1080x1920; 1e-9 is six orders above that, six below the third decimal evals.py prints, and an fp32
  evaluation of S (error near 1e-6) cannot pass it.
* histogram matching: bit for bit (int32 view), no tolerance, no excluded elements."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_TOL = 1e-9


# ------------------------------------------------------------------------------------------------------------- references
def ssim_ref(a_u8, b_u8):
    """skimage.metrics.structural_similarity(a, b, channel_axis=2, data_range=255) on HWC uint8 (gaussian_weights=False)."""
    from scipy.ndimage import uniform_filter
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    cov_norm = 49.0 / 48.0
    per_channel = []
    for c in range(a_u8.shape[2]):
        x, y = a_u8[..., c].astype(np.float64), b_u8[..., c].astype(np.float64)
        ux, uy = uniform_filter(x, size=7), uniform_filter(y, size=7)
        uxx, uyy, uxy = uniform_filter(x * x, size=7), uniform_filter(y * y, size=7), uniform_filter(x * y, size=7)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        per_channel.append(S[3:-3, 3:-3].mean(dtype=np.float64))
    return float(np.mean(per_channel))


def hm_ref(src, tmpl):
    """skimage.exposure.match_histograms(src, tmpl) with channel_axis=None on float input (_match_cumulative_cdf)."""
    _, inv, sc = np.unique(src.ravel(), return_inverse=True, return_counts=True)
    tv, tc = np.unique(tmpl.ravel(), return_counts=True)
    sq = np.cumsum(sc) / src.size
    tq = np.cumsum(tc) / tmpl.size
    return np.interp(sq, tq, tv)[inv.ravel()].reshape(src.shape).astype(np.float32)


def u8_hwc(x):
    """[1,3,H,W] float32 -> HWC uint8 the way evals.py:83-84 quantises"""
    return np.round(x[0].transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)


def levels_image(rng, shape, lo=0, hi=256):
    """a ToTensor image: float32(k) / 255 with k uniform in [lo, hi)"""
    return rng.integers(lo, hi, size=shape).astype(np.float32) / np.float32(255)


# ------------------------------------------------------------------------------------------------------------- parametrisation
def _backend_size_cases(small, large):
    """every size on the MI355X, only the small ones in the host emulator (the large ones are never collected for it)"""
    out = []
    for (h, w) in small:
        out.append(pytest.param("emu", (h, w), id="emu-%dx%d" % (h, w)))
    for (h, w) in list(small) + list(large):
        out.append(pytest.param("hip", (h, w), id="hip-%dx%d" % (h, w), marks=pytest.mark.gpu))
    return out


SSIM_CASES = _backend_size_cases([(7, 7), (30, 44), (37, 53)], [(270, 480), (1080, 1920)])
HM_CASES = _backend_size_cases([(16, 16), (37, 53), (64, 96)], [(270, 480), (1080, 1920)])


def _ssim_pair(kind, synth, H, W):
    rng = np.random.default_rng(1000 + H * 7 + W)
    if kind == "lowlight":
        a = np.clip(synth.lowlight_frame(0, H, W) * np.float32(3), np.float32(1e-4), np.float32(1)).astype(np.float32)
        clean = np.asarray(synth.clean_frame(0, H, W), dtype=np.float32).reshape(1, 3, H, W)
        b = (np.round(clean * np.float32(255)) / np.float32(255)).astype(np.float32)
    elif kind == "random":
        a, b = rng.random((1, 3, H, W), dtype=np.float32), rng.random((1, 3, H, W), dtype=np.float32)
    elif kind == "self":
        a = rng.random((1, 3, H, W), dtype=np.float32)
        b = a.copy()
    else:
        a = np.full((1, 3, H, W), 0.3, np.float32)
        b = np.full((1, 3, H, W), 0.7, np.float32)
    return a, b


# ------------------------------------------------------------------------------------------------------------- SSIM
@pytest.mark.parametrize("kind", ["lowlight", "random", "self", "const"])
@pytest.mark.parametrize("backend,size", SSIM_CASES, indirect=["backend"])
def test_ssim_parity(backend, synth, size, kind):
    ops, dev, _ = backend
    H, W = size
    a, b = _ssim_pair(kind, synth, H, W)
    ours = ops.ssim_u8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    ref = ssim_ref(u8_hwc(a), u8_hwc(b))
    print("ssim %s %dx%d: ours %.17g ref %.17g |d| %.3g" % (kind, H, W, ours, ref, abs(ours - ref)))
    assert abs(ours - ref) <= SSIM_TOL, (ours, ref)
    if kind == "self":
        assert ours == 1.0


def test_ssim_deterministic(backend, synth):
    ops, dev, _ = backend
    a, b = _ssim_pair("random", synth, 37, 53)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert ops.ssim_u8(ta, tb) == ops.ssim_u8(ta, tb)


def test_ssim_refuses_small_frames(backend):
    ops, dev, _ = backend
    for H, W in ((6, 32), (32, 6)):
        x = torch.zeros((1, 3, H, W), dtype=torch.float32, device=dev)
        with pytest.raises(RuntimeError, match="1001"):
            ops.ssim_u8(x, x)


# ------------------------------------------------------------------------------------------------------------- histogram matching
def _hm_case(kind, H, W):
    rng = np.random.default_rng(77 + H * 13 + W)
    shape = (1, 3, H, W)
    src = rng.random(shape, dtype=np.float32)
    tmpl = levels_image(rng, shape)
    if kind == "ties":
        src = (np.round(src * np.float32(64)) / np.float32(64)).astype(np.float32)
    elif kind == "signed":
        src = (src - np.float32(0.5)).astype(np.float32)
        flat = src.reshape(-1)
        idx = rng.choice(flat.size, size=min(12, flat.size // 4), replace=False)
        flat[idx[0::2]] = np.float32(-0.0)
        flat[idx[1::2]] = np.float32(0.0)
    elif kind == "const":
        src = np.full(shape, 0.37, np.float32)
    elif kind == "one_level":
        tmpl = np.full(shape, np.float32(128) / np.float32(255), np.float32)
    elif kind == "small_tmpl":
        tmpl = levels_image(rng, (1, 3, 9, 11))
    elif kind == "band":
        tmpl = levels_image(rng, shape, 40, 90)
    else:
        assert kind == "uniform"
    return src, tmpl


def _assert_bits(ours, ref):
    assert ours.dtype == torch.float32 and tuple(ours.shape) == ref.shape
    assert torch.equal(ours.cpu().view(torch.int32), torch.from_numpy(ref).view(torch.int32)), \
        "%d of %d elements differ" % (int((ours.cpu().view(torch.int32) != torch.from_numpy(ref).view(torch.int32)).sum()), ref.size)


@pytest.mark.parametrize("kind", ["uniform", "ties", "signed", "const", "one_level", "small_tmpl", "band"])
@pytest.mark.parametrize("backend,size", HM_CASES, indirect=["backend"])
def test_match_histograms_bit_exact(backend, size, kind):
    ops, dev, _ = backend
    H, W = size
    src, tmpl = _hm_case(kind, H, W)
    ours = ops.match_histograms(torch.from_numpy(src).to(dev), torch.from_numpy(tmpl).to(dev))
    assert ours.device.type == dev.type
    _assert_bits(ours, hm_ref(src, tmpl))


def test_match_histograms_pools_channels(backend):
    """skimage's default channel_axis=None (what the reference calls) matches ONE distribution over all three channels."""
    ops, dev, _ = backend
    rng = np.random.default_rng(5)
    H, W = 37, 53
    src = np.stack([rng.random((H, W), dtype=np.float32) * np.float32(0.3) + np.float32(off) for off in (0.0, 0.35, 0.7)])[None]
    tmpl = levels_image(rng, (1, 3, H, W))
    pooled = hm_ref(src, tmpl)
    per_channel = np.stack([hm_ref(src[0, c], tmpl[0, c]) for c in range(3)])[None]
    assert not np.array_equal(pooled, per_channel)
    ours = ops.match_histograms(torch.from_numpy(src).to(dev), torch.from_numpy(tmpl).to(dev))
    _assert_bits(ours, pooled)
    assert not np.array_equal(ours.cpu().numpy(), per_channel)


def test_metrics_after_matching(backend):
    ops, dev, _ = backend
    rng = np.random.default_rng(9)
    H, W = 37, 53
    src = rng.random((1, 3, H, W), dtype=np.float32)
    gt = levels_image(rng, (1, 3, H, W))
    gt_d = torch.from_numpy(gt).to(dev)
    hm = ops.match_histograms(torch.from_numpy(src).to(dev), gt_d)
    ref = hm_ref(src, gt)
    a_u8, g_u8 = u8_hwc(ref), u8_hwc(gt)
    sq = int(((a_u8.astype(np.int64) - g_u8.astype(np.int64)) ** 2).sum())
    assert sq > 0
    assert ops.psnr_u8(hm, gt_d) == 10.0 * math.log10(255.0 ** 2 * src.size / sq)
    ours, want = ops.ssim_u8(hm, gt_d), ssim_ref(a_u8, g_u8)
    print("ssim after matching: ours %.17g ref %.17g" % (ours, want))
    assert abs(ours - want) <= SSIM_TOL


# ------------------------------------------------------------------------------------------------------------- evals.py
@pytest.mark.gpu
def test_evals_script_reports_ssim_and_histogram_matched_metrics(tmp_path, synth):
    """evals.py end to end on a four-frame BVI-RLV-layout clip with a randomly initialised model: every metric of Metrics.json but
    LPIPS is a finite number, the matched frames are written, and --hist_match 0 leaves the plain metrics untouched (the two
    child processes agree to the last bit because evals.py seeds the RAFT that Finetunemodel draws after reading the weights)."""
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
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run_evals(save, *extra):
        r = subprocess.run([sys.executable, "evals.py", "--dataset", "RLV", "--lowlight_images_path", str(data), "--model_pretrain",
                            str(weights), "--save", str(save)] + list(extra), cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        return json.load(open(save / "Metrics.json")), r.stdout

    m, out = run_evals(tmp_path / "ev")
    print(m)
    for k in ("Total_PSNR", "Total_SSIM", "Total_PSNR_HM", "Total_SSIM_HM"):
        assert isinstance(m[k], float) and math.isfinite(m[k]), (k, m)
    assert -1.0 <= m["Total_SSIM"] <= 1.0 and -1.0 <= m["Total_SSIM_HM"] <= 1.0
    assert m["Total_LPIPS"] is None and m["Total_LPIPS_HM"] is None and m["images"] == 4
    assert len(list((tmp_path / "ev").rglob("*_denoise_hm.png"))) == 4
    assert len(list((tmp_path / "ev").rglob("*_denoise.png"))) == 4
    assert "SSIM_HM:" in out and "Total PSNR_HM:" in out

    m0, _ = run_evals(tmp_path / "ev0", "--hist_match", "0")
    assert m0["Total_PSNR"] == m["Total_PSNR"] and m0["Total_SSIM"] == m["Total_SSIM"]
    assert m0["Total_PSNR_HM"] is None and m0["Total_SSIM_HM"] is None and m0["images"] == 4
    assert len(list((tmp_path / "ev0").rglob("*_denoise_hm.png"))) == 0
