"""evals.py --y4m_in LOW --y4m_gt GT: the argument checks on the CPU, the video mode end to end on the MI355X.

End to end the script is held against three things it does not compute itself: predict.py's `_denoise.y4m` of the same low stream
(same seed, same weights) and the ground-truth file, read back with numpy, for the plane metrics -- the integer SSEs must be equal,
PSNR must follow from them by the formula, SSIM_Y must sit within SSIM_TOL of the reference of tests/test_planes.py on those files;
and an InferStep of the test's own, graded frame by frame through `utils.psnr` / `utils.ssim`, for Total_PSNR / Total_SSIM (equal:
the same kernels on the same bits, added in the same order)."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_metrics import SSIM_TOL
from test_planes import ssim_plane_ref

H, W, FRAMES = 128, 160, 5
CUT_AT = 5                                                  # the spliced clip: frames 0-4 of seed 2, frames 5-8 of seed 7
THRESHOLD = 0.04


def _y4m():
    return importlib.import_module("zero-tig_amd.y4m")


def _run(script, *args, ok=True):
    r = subprocess.run([sys.executable, script] + [str(a) for a in args], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r


def _frames_of(path):
    r = _y4m().Y4MReader(str(path), pin=False)
    return r.header, [f.numpy().copy() for f in r]


def _payloads(synth, fmt, frames, clean):
    """[(frame index, seed)] -> payloads of `fmt` from the synthetic low-light clip or its clean twin"""
    y, out = _y4m(), []
    for t, seed in frames:
        a = np.asarray((synth.clean_frame if clean else synth.lowlight_frame)(t, fmt.H, fmt.W, seed), dtype=np.float32)
        chw = a[0] if a.ndim == 4 else a
        if fmt.depth > 8:
            rgb = (np.transpose(chw, (1, 2, 0)).astype(np.float64) * 65535.0 + 0.5).astype(np.uint16)
        else:
            rgb = (np.transpose(chw, (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
        out.append(y.encode_host(rgb, fmt))
    return out


def _write(path, head, payloads):
    _y4m().write_file(str(path), head, payloads)
    return path


def _weights(tmp_path, synth):
    path = tmp_path / "weights.pt"
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, str(path))
    return path


# ------------------------------------------------------------------------------------------------- argument checks (no device)
@pytest.mark.parametrize("extra,words", [
    (("--y4m_gt", "GT"), ("--y4m_gt", "needs --y4m_in")),
    (("--y4m_in", "LOW"), ("--y4m_in", "needs --y4m_gt")),
    (("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "0"), ("--y4m_in needs --graph 1", "--graph is 0")),
    (("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "1", "--device_png", "1"), ("--device_png 1 cannot be combined",)),
    (("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "1", "--save_images", "3"), ("--save_images cannot be combined",)),
    (("--y4m_in", "LOW", "--y4m_gt", "-", "--graph", "1"), ("--y4m_gt must be a file",)),
    (("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "1", "--y4m_size", "1920"), ("--y4m_size takes WxH", "'1920'")),
    (("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "1", "--y4m_size", "axb"), ("--y4m_size takes WxH",)),
    (("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "1", "--y4m_cuts_json", "C"), ("--y4m_cuts_json needs --y4m_scene_cut",)),
    (("--y4m_in", "LOW", "--y4m_gt", "MISSING", "--graph", "1"), ("MISSING: no such file",)),
], ids=["gt-alone", "in-alone", "graph0", "device_png", "save_images", "gt-stdin", "size-1920", "size-axb", "cuts_json-alone", "gt-missing"])
def test_argument_checks(tmp_path, extra, words):
    """every check runs before anything touches the device (this machine has none) and before --save is created"""
    (tmp_path / "LOW").write_bytes(b"")
    if "MISSING" not in extra:
        (tmp_path / "GT").write_bytes(b"")
    extra = [str(tmp_path / a) if a in ("LOW", "GT", "MISSING", "C", "F") else a for a in extra]
    r = _run("evals.py", "--save", tmp_path / "out", *extra, ok=False)
    assert r.returncode == 2, (r.returncode, r.stderr[-800:])
    for w in words:
        assert w in r.stderr, (w, r.stderr[-800:])
    assert not (tmp_path / "out").exists()


# ----------------------------------------------------------------------------------------------------------- end to end
def _plane_sse(fmt, a, b):
    m = (1 << fmt.depth) - 1
    return [int(((np.minimum(x.astype(np.int64), m) - np.minimum(y.astype(np.int64), m)) ** 2).sum())
            for x, y in zip(fmt.planes(a), fmt.planes(b))]


def _own_rgb_metrics(evals_argv, low, fmt, gt, gt_fmt):
    """Total_PSNR / Total_SSIM the way the PNG loop of evals.py adds them up, from an InferStep of the test's own"""
    evals = importlib.import_module("evals")
    utils = evals.utils
    args = evals.parser.parse_args([str(a) for a in evals_argv])
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", 0)
    model = evals.Finetunemodel(args).to(dev)
    model.eval()
    for p in model.parameters():
        p.requires_grad = False
    step = importlib.import_module("zero-tig_amd.infer").InferStep(model, use_graph=True, ingest_size=None, yuv=fmt, yuv_out_depth=fmt.depth)
    ops = utils._ops()
    total, total_ssim = 0.0, 0.0
    with torch.no_grad():
        for t, (p, g) in enumerate(zip(low, gt)):
            _, output, _ = step(torch.from_numpy(p.copy()).pin_memory(), t == 0)
            gt_t = ops.yuv_to_planar_f32(torch.from_numpy(g.copy()).to(dev), gt_fmt)
            total += utils.psnr(output, gt_t)
            total_ssim += utils.ssim(output, gt_t)
    return total / len(low), total_ssim / len(low)


@pytest.mark.gpu
@pytest.mark.parametrize("ctag,color_range", [("420mpeg2", "LIMITED"), ("444p10", None)])
def test_evals_y4m_end_to_end(tmp_path, synth, ctag, color_range):
    head = _y4m().Header(W, H, "25:1", "p", None, ctag, color_range)
    fmt = head.format("bt709")
    frames = [(t, 2) for t in range(FRAMES)]
    low, gt = _payloads(synth, fmt, frames, False), _payloads(synth, fmt, frames, True)
    src, ref = _write(tmp_path / "low.y4m", head, low), _write(tmp_path / "gt.y4m", head, gt)
    common = ("--model_pretrain", _weights(tmp_path, synth), "--graph", "1", "--precision", "bf16", "--of_scale", "1", "--y4m_in", src)
    _run("predict.py", *common, "--save", tmp_path / "pred")
    fj = tmp_path / "frames.json"
    ev_args = common + ("--y4m_gt", ref, "--save", tmp_path / "ev", "--y4m_frames_json", fj, "--y4m_out", tmp_path / "enh.y4m")
    r = _run("evals.py", *ev_args)
    m, rec = json.load(open(str(tmp_path / "ev" / "Metrics.json"))), json.load(open(str(fj)))
    print(m)

    # the plane metrics against predict.py's denoise stream and the ground-truth file, read back with numpy
    dh, den = _frames_of(tmp_path / "pred" / "low_denoise.y4m")
    gh, gts = _frames_of(ref)
    assert dh == head and gh == head and len(den) == FRAMES and len(gts) == FRAMES
    sse = [_plane_sse(fmt, d, g) for d, g in zip(den, gts)]
    assert len(rec) == FRAMES and [f["SSE"] for f in rec] == sse and [f["frame"] for f in rec] == list(range(FRAMES))
    pl = m["planes"]
    hc, wc = fmt.chroma_shape
    assert pl["depth"] == fmt.depth and pl["ss"] == fmt.ss and pl["samples"] == [H * W, hc * wc, hc * wc]
    assert pl["SSE"] == [sum(s[p] for s in sse) for p in range(3)] and all(v > 0 for v in pl["SSE"])
    peak = (1 << fmt.depth) - 1
    for p, name in enumerate("YUV"):
        assert pl["PSNR_" + name] == 10.0 * math.log10(peak * peak * pl["samples"][p] * FRAMES / pl["SSE"][p])
        per_frame = [ssim_plane_ref(fmt.planes(d)[p], fmt.planes(g)[p], peak) for d, g in zip(den, gts)]
        for f, want in zip(rec, per_frame):
            assert abs(f["SSIM_" + name] - want) <= SSIM_TOL, (name, f["frame"], f["SSIM_" + name], want)
        assert abs(pl["SSIM_" + name] - sum(per_frame) / FRAMES) <= SSIM_TOL
    # --y4m_out: the enhance stream predict.py writes
    assert (tmp_path / "enh.y4m").read_bytes() == (tmp_path / "pred" / "low_enhance.y4m").read_bytes()

    # the RGB metrics against an InferStep of the test's own, graded through utils.psnr / utils.ssim
    psnr, ssim = _own_rgb_metrics(ev_args, low, fmt, gt, fmt)
    assert m["Total_PSNR"] == psnr and m["Total_SSIM"] == ssim, (m["Total_PSNR"], psnr, m["Total_SSIM"], ssim)
    assert m["Total_PSNR"] == sum(f["PSNR"] for f in rec) / FRAMES and m["Total_SSIM"] == sum(f["SSIM"] for f in rec) / FRAMES
    for k in ("Total_PSNR_HM", "Total_SSIM_HM"):
        assert isinstance(m[k], float) and math.isfinite(m[k]), (k, m)
    assert m["Total_LPIPS"] is None and m["Total_LPIPS_HM"] is None and m["images"] == FRAMES and "cuts" not in m
    assert all(f["cut"] is False for f in rec)
    assert sum(line.split(" ", 3)[-1].startswith("NUM: %d, PSNR: " % FRAMES) for line in r.stdout.split("\n")) == 1, r.stdout[-2000:]
    assert "PSNR_HM:" in r.stdout and "SSIM_Y:" in r.stdout


@pytest.mark.gpu
def test_evals_y4m_other_layout_and_scene_cut(tmp_path, synth):
    """a ground truth of another subsampling and depth still grades the RGB frames (planes: null, one log line says why), and a
    low stream spliced from two scenes reports the cut at the splice"""
    y = _y4m()
    head, gt_head = y.Header(W, H, "25:1", "p", None, "420mpeg2", "LIMITED"), y.Header(W, H, "25:1", "p", None, "444p10", None)
    frames = [(t, 2 if t < CUT_AT else 7) for t in range(9)]
    low = _payloads(synth, head.format("bt709"), frames, False)
    gt = _payloads(synth, gt_head.format("bt709"), frames, True)
    src, ref = _write(tmp_path / "low.y4m", head, low), _write(tmp_path / "gt.y4m", gt_head, gt)
    fj, cj = tmp_path / "frames.json", tmp_path / "cuts.json"
    r = _run("evals.py", "--model_pretrain", _weights(tmp_path, synth), "--graph", "1", "--precision", "bf16", "--of_scale", "1",
             "--y4m_in", src, "--y4m_gt", ref, "--save", tmp_path / "ev", "--hist_match", "0", "--y4m_scene_cut", THRESHOLD,
             "--y4m_cuts_json", cj, "--y4m_frames_json", fj)
    m, rec, cuts = (json.load(open(str(p))) for p in (tmp_path / "ev" / "Metrics.json", fj, cj))
    assert m["planes"] is None and m["images"] == 9 and m["cuts"] == [CUT_AT] and cuts["cuts"] == [CUT_AT]
    assert [f["cut"] for f in rec] == [t == CUT_AT for t in range(9)]
    assert all(f["SSE"] is None and f["SSIM_Y"] is None for f in rec)
    assert math.isfinite(m["Total_PSNR"]) and -1.0 <= m["Total_SSIM"] <= 1.0
    assert m["Total_PSNR_HM"] is None and m["Total_SSIM_HM"] is None
    assert sum("plane metrics off" in line for line in r.stdout.split("\n")) == 1, r.stdout[-2000:]
    assert sum("scene cut at frame %d" % CUT_AT in line for line in r.stdout.split("\n")) == 1


@pytest.mark.gpu
def test_evals_y4m_ground_truth_one_frame_short(tmp_path, synth):
    head = _y4m().Header(W, H, "25:1", "p", None, "420mpeg2", "LIMITED")
    fmt = head.format("bt709")
    frames = [(t, 2) for t in range(FRAMES)]
    src = _write(tmp_path / "low.y4m", head, _payloads(synth, fmt, frames, False))
    ref = _write(tmp_path / "gt.y4m", head, _payloads(synth, fmt, frames[:-1], True))
    r = _run("evals.py", "--model_pretrain", _weights(tmp_path, synth), "--graph", "1", "--precision", "bf16", "--of_scale", "1",
             "--y4m_in", src, "--y4m_gt", ref, "--save", tmp_path / "ev", "--hist_match", "0", ok=False)
    assert r.returncode != 0 and "--y4m_in has %d frames, --y4m_gt has %d" % (FRAMES, FRAMES - 1) in r.stderr, r.stderr[-1500:]
    assert not (tmp_path / "ev" / "Metrics.json").exists()
