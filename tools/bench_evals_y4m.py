#!/usr/bin/env python3
"""GPU box: what grading a raw video costs (evals.py --y4m_in / --y4m_gt).  One MI355X, at most 16 CPUs.

(a) kernels: HIP-event median over --reps calls of the two entry points of zt_planes.hip alone on a 1080p C420 pair, at 8 and at
    10 bits: `Ops.yuv_sse` on the whole payloads, `Ops.ssim_plane` on the luma plane and on one chroma plane, each with 16-byte
    loads and, from a payload one sample off a 16-byte boundary, with sample-wide loads; the bytes each call reads and the rate.
(b) end to end: a synthetic 1080p C420mpeg2 pair (--frames frames, --distinct different ones; low-light and clean twin of
    zero-tig_amd/synth.py through the host encoder of zero-tig_amd/y4m.py), --repeats runs each, the runs of the settings alternating:
      predict        predict.py --graph 1 --precision bf16 --y4m_in LOW (two Y4M streams written): the loop evals.py extends
      evals          evals.py   --graph 1 --precision bf16 --y4m_in LOW --y4m_gt GT --hist_match 0 (PSNR, SSIM, the plane metrics)
      evals_hm       the same with histogram matching on (PSNR_HM, SSIM_HM)
      evals_lpips    the same as `evals` with --lpips_weights (synthetic VGG weights, seeded) --lpips_precision bf16
      evals_tc3      the same as `evals` with --tc 1 --tc_scale 3 (temporal consistency at 360 x 640)
      evals_tc1      the same with --tc_scale 1 (at 1080 x 1920)
    frames per second and the host-side split per frame from each script's --timing_json.
(c) the temporal kernel: HIP-event median over --reps calls of `Ops.warp_error` at 360 x 640 and 1080 x 1920, next to `Ops.warp2`
    (the same gather pattern) and to one RAFT run of `TemporalConsistency` at the same sizes.

(d) no reference: `evals_noref` = evals.py --y4m_in LOW --noref 1 in part (b), and the two entry points of zt_noref.hip
    alone at 1080p -- the joint histogram on the full grid, `zt_noref_from_hist`, `Ops.noref` on the full and on the LOE_50 grid --
    next to `Ops.ssim_u8_dev` in the same process, on four inputs: the synthetic low-light frame against its clean twin, 13 dark
    levels against noise, one bin (two constant frames) and uniform noise.  `--settings evals_noref --skip-kernels --skip-temporal
    --out profiles/noref_1080p.json` is the run behind that file.

(e) the pictures of --tc 1: `evals_tcviz` = `evals_tc3` with --tc_viz and --tc_flo_dir (a 1280 x 720 stream and two
    .flo files per pair written), `evals_tcviz_pic` = with --tc_viz alone; the yardstick is `evals_tc3` in the same run
    (`tcviz_over_tc3_ms_per_frame`).  With either, the kernels of zt_flowviz.hip alone at 360 x 640: `Ops.tc_viz` with the bytes it
    moves, `Ops.flow_radmax` of two flows, `Ops.flow_pack`, and `Ops.rgb_f32_to_yuv` of the picture.  `--settings evals_tc3
    evals_tcviz_pic evals_tcviz --skip-kernels --skip-temporal --frames 128 --out profiles/evals_tcviz_1080p.json` is the run behind
    that file.

(f) colour: `evals_color` = `evals_noref` with --color 1 in part (b), and `Ops.color_stats` alone at 1080p on four
    inputs (the low-light frame, its clean twin, a constant frame, uniform noise), at the default grid and at three others, with
    blocks of 10, 8 and 64, next to `Ops.ssim_u8_dev` in the same process.  `--settings evals_noref evals_color --skip-kernels
    --skip-temporal --frames 128 --out profiles/color_1080p.json` is the run behind that file.

(g) NIQE: `evals_niqe` = `evals_noref` with --niqe MODEL in part (b); the model is fitted first by tools/niqe_fit.py
    from every 16th frame of the ground-truth clip.  And the two kernels alone at 1080p on three inputs (the low-light frame, its
    clean twin, uniform noise): `Ops.niqe_block_sums`, `Ops.niqe_frame_from_sums`, both as `Ops.niqe_frame`, next to a plain-torch
    composition of the same definition on the device (index gather and `F.conv2d` for the half-size image, `F.pad` / `F.conv2d` for
    the window, `torch.roll` for the products, the fits by `torch.searchsorted`, `torch.cov`) and to `Ops.ssim_u8_dev`.
    `--settings evals_noref evals_niqe --skip-kernels --skip-temporal --frames 128 --out profiles/niqe_1080p.json` is the run
    behind that file.

This driver never opens the GPU itself: every GPU step is a child process under its own `timeout -k 10`, and the first failure
ends the run.  Writes the JSON to --out and prints it as one line.
Usage: python tools/bench_evals_y4m.py [--frames 256] [--out profiles/evals_y4m_1080p.json]"""
import argparse
import importlib
import json
import math
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 1080, 1920


# ---- child: the two entry points alone -------------------------------------------------------------------------------------------
def kernels_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    y4m = importlib.import_module("zero-tig_amd.y4m")
    out = {"format": "1080x1920 C420, limited, bt709: payloads of the low-light frame 3 (x 4, clipped) and its clean twin"}
    low = np.clip(np.transpose(np.asarray(synth.lowlight_frame(3, H, W))[0], (1, 2, 0)).astype(np.float64) * 4.0, 0.0, 1.0)
    clean = np.transpose(np.asarray(synth.clean_frame(3, H, W)).reshape(3, H, W), (1, 2, 0)).astype(np.float64)

    def shifted(p, es):                             # the same bytes one sample behind a 16-byte boundary
        buf = torch.empty(p.numel() + 16, dtype=torch.uint8, device="cuda")
        view = buf[es:es + p.numel()]
        view.copy_(p)
        return view
    for depth in (8, 10):
        fmt = y4m.YuvFormat(W, H, 420, 1, "bt709", 0, depth)
        if depth == 8:
            pay = [y4m.encode_host((x * 255.0 + 0.5).astype(np.uint8), fmt) for x in (low, clean)]
        else:
            pay = [y4m.encode_host((x * 65535.0 + 0.5).astype(np.uint16), fmt) for x in (low, clean)]
        es = 2 if depth > 8 else 1
        pa, pb = (torch.from_numpy(p).cuda() for p in pay)
        sa, sb = shifted(pa, es), shifted(pb, es)
        sse3 = torch.empty(3, dtype=torch.int64, device="cuda")
        one = torch.empty(1, dtype=torch.float64, device="cuda")
        hc, wc = fmt.chroma_shape
        calls = {"yuv_sse": (lambda: ops.yuv_sse(pa, pb, fmt, out=sse3), 2 * fmt.frame_bytes),
                 "yuv_sse_sample_loads": (lambda: ops.yuv_sse(sa, sb, fmt, out=sse3), 2 * fmt.frame_bytes),
                 "ssim_plane_Y": (lambda: ops.ssim_plane(pa, pb, fmt, 0, out=one), 2 * es * H * W),
                 "ssim_plane_Y_sample_loads": (lambda: ops.ssim_plane(sa, sb, fmt, 0, out=one), 2 * es * H * W),
                 "ssim_plane_U": (lambda: ops.ssim_plane(pa, pb, fmt, 1, out=one), 2 * es * hc * wc)}
        row = {"payload_bytes": fmt.frame_bytes}
        for name, (fn, read) in calls.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            row[name] = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes_read": read,
                         "gbs": round(read / med / 1e6, 1)}
            print("[bench_evals_y4m] %d-bit %s %s" % (depth, name, row[name]), file=sys.stderr, flush=True)
        ref = ops.yuv_sse(pa, pb, fmt).tolist()
        assert ops.yuv_sse(sa, sb, fmt).tolist() == ref, "the sample-wide and the 16-byte path disagree"
        assert ops.ssim_plane(pa, pb, fmt, 0).item() == ops.ssim_plane(sa, sb, fmt, 0).item()
        m = (1 << depth) - 1
        row["sse"] = ref
        row["psnr_y"] = 10.0 * math.log10(m * m * H * W / ref[0])
        row["ssim_y"] = ops.ssim_plane(pa, pb, fmt, 0).item()
        out["depth_%d" % depth] = row
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- child: the temporal kernel alone, next to zt_warp2_f32 and to the RAFT runs that feed it -----------------------------
def temporal_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    temporal = importlib.import_module("zero-tig_amd.temporal")
    dev = torch.device("cuda", 0)
    weights = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in synth.make_state(3).items() if k.startswith("raft.")}

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)
    out = {"what": "HIP-event median of %d calls: Ops.warp_error (one frame pair, flows at the frame's size), Ops.warp2 (two 3-channel "
                   "images, flow at the frame's size) and one RAFT run of TemporalConsistency (bf16, 12 iterations); bytes = every "
                   "array read or written once" % a.reps}
    for h, w in ((360, 640), (1080, 1920)):
        def frame(fn, t):
            return torch.from_numpy(np.ascontiguousarray(np.asarray(fn(t, h, w), dtype=np.float32).reshape(1, 3, h, w))).to(dev)
        cur, prev = frame(synth.lowlight_frame, 4), frame(synth.lowlight_frame, 3)
        gcur, gprev = frame(synth.clean_frame, 4), frame(synth.clean_frame, 3)
        tc = temporal.TemporalConsistency(ops, weights, dev, h, w, 1, "bf16")
        g1, g0 = gcur * 255.0, gprev * 255.0
        fb, ff = tc.flow(g1, g0), tc.flow(g0, g1)
        on, o3 = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
        row = {}
        for name, fn, nbytes in (("warp_error", lambda: ops.warp_error(cur, prev, fb, ff, out_n=on, out3=o3), 40 * h * w),
                                 ("warp2", lambda: ops.warp2(fb, prev, gprev), 56 * h * w),
                                 ("raft_flow", lambda: tc.flow(g1, g0), None)):
            med, lo, hi = timed(fn)
            row[name] = {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
            if nbytes is not None:
                row[name].update(bytes=nbytes, gbs=round(nbytes / med / 1e6, 1))
            print("[bench_evals_y4m] %dx%d %s %s" % (h, w, name, row[name]), file=sys.stderr, flush=True)
        row["valid_share"] = int(on.item()) / (h * w)
        row["sums"] = o3.tolist()
        out["%dx%d" % (h, w)] = row
        del tc, fb, ff
        torch.cuda.empty_cache()
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- child: the two entry points of zt_noref.hip alone, next to zt_ssim_u8_f32 ----------------------------------------------
def noref_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)

    def dev_frame(x):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(1, 3, H, W))).to(dev)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    inputs = {"synth_lowlight": (dev_frame(synth.lowlight_frame(3, H, W)), dev_frame(synth.clean_frame(3, H, W))),
              "dark_13_levels": (dev_frame(rng.integers(0, 13, (3, H, W)) / np.float32(255)), dev_frame(rng.random((3, H, W), dtype=np.float32))),
              "one_bin": (torch.full((1, 3, H, W), 0.02, device=dev), torch.full((1, 3, H, W), 0.5, device=dev)),
              "uniform_noise": (dev_frame(rng.random((3, H, W), dtype=np.float32)), dev_frame(rng.random((3, H, W), dtype=np.float32)))}
    grid50 = (50, 89)
    out = {"what": "HIP-event median of %d calls at 1080 x 1920: hist = zt_lightness_joint_hist_f32 on the full grid (the memset of the "
                   "table included; it reads both frames once, bytes = 24 H W), from_hist = zt_noref_from_hist, noref / noref_50 = "
                   "Ops.noref (both kernels) on the full grid / on the 50 x 89 grid, ssim_u8 = Ops.ssim_u8_dev on the same frames" % a.reps}
    for name, (x, y) in inputs.items():
        hist = torch.empty((256, 256), dtype=torch.uint32, device=dev)
        oi, of = torch.empty(6, dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.float64, device=dev)
        one = torch.empty(1, dtype=torch.float64, device=dev)
        row = {"hist": timed(lambda: ops.lightness_joint_hist(x, y, out=hist))}
        row["hist"].update(bytes=24 * H * W, gbs=round(24 * H * W / row["hist"]["ms"] / 1e6, 1))
        row["from_hist"] = timed(lambda: lib.call("zt_noref_from_hist", hist, oi, of, ops._s(x)))
        row["noref"] = timed(lambda: ops.noref(x, y, out_i=oi, out_f=of))
        row["noref_50"] = timed(lambda: ops.noref(x, y, grid=grid50, out_i=oi, out_f=of))
        row["ssim_u8"] = timed(lambda: ops.ssim_u8_dev(x, y, out=one))
        ops.noref(x, y, out_i=oi, out_f=of)
        h = hist.cpu().numpy()
        row.update(occupied_bins=int((h != 0).sum()), occupied_La_levels=int((h.sum(axis=1) != 0).sum()), ints=oi.tolist(), entropies=of.tolist())
        out[name] = row
        print("[bench_evals_y4m] noref %s %s" % (name, row), file=sys.stderr, flush=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- child: zt_color_stats_f32 alone, next to zt_ssim_u8_f32 ----------------------------------------------------------------
def color_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    grading = importlib.import_module("zero-tig_amd.grading")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)

    def dev_frame(x):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(1, 3, H, W))).to(dev)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    inputs = {"synth_lowlight": dev_frame(synth.lowlight_frame(3, H, W)), "synth_clean": dev_frame(synth.clean_frame(3, H, W)),
              "constant": torch.full((1, 3, H, W), 0.25, device=dev), "uniform_noise": dev_frame(rng.random((3, H, W), dtype=np.float32))}
    out = {"what": "HIP-event median of %d calls at 1080 x 1920: color = Ops.color_stats, blocks of 10 (the memset of the table, the "
                   "pass over the frame and the finishing workgroup; it reads the frame once, bytes = 12 H W), color_wgN = the same "
                   "with max_workgroups = N (the default grid is 216 workgroups here, one unit each), color_b8 / color_b64 = blocks of 8 / 64, "
                   "ssim_u8 = Ops.ssim_u8_dev of the frame against the clean frame, in the same process" % a.reps}
    for name, x in inputs.items():
        oi, of = torch.empty(18, dtype=torch.int64, device=dev), torch.empty(7, dtype=torch.float64, device=dev)
        one = torch.empty(1, dtype=torch.float64, device=dev)
        row = {"color": timed(lambda: ops.color_stats(x, 10, out_i=oi, out_f=of))}
        row["color"].update(bytes=12 * H * W, gbs=round(12 * H * W / row["color"]["ms"] / 1e6, 1))
        for wg in (27, 54, 108):
            row["color_wg%d" % wg] = timed(lambda: ops.color_stats(x, 10, out_i=oi, out_f=of, max_workgroups=wg))
        for b in (8, 64):
            row["color_b%d" % b] = timed(lambda: ops.color_stats(x, b, out_i=oi, out_f=of))
        row["ssim_u8"] = timed(lambda: ops.ssim_u8_dev(x, inputs["synth_clean"], out=one))
        ops.color_stats(x, 10, out_i=oi, out_f=of)
        row.update(ints=oi.tolist(), sums=of.tolist(), values=grading.color_values(oi.tolist(), of.tolist(), 10))
        out[name] = row
        print("[bench_evals_y4m] color %s %s" % (name, row), file=sys.stderr, flush=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- child: the two kernels of zt_niqe.hip alone, next to a plain-torch composition of the same definition -----------------
def torch_niqe(x, win, r_gam, c1, c2):
    """the definition of include/zerotig_hip.h in plain torch on the device -> (column sums over finite, counts, nv, mean of the
    valid rows, their covariance); float32 per pixel, float64 sums, as the kernels"""
    import torch
    import torch.nn.functional as F
    Hc, Wc = x.shape[2] // 96 * 96, x.shape[3] // 96 * 96
    lv = torch.round(x[0] * 255.0).to(torch.int64) & 255
    g = ((19591 * lv[0] + 38472 * lv[1] + 7473 * lv[2] + 32768) >> 16)[:Hc, :Wc].to(torch.float32)

    def sym(n):                                     # indices -3 .. n + 3, reflected with the edge repeated
        i = torch.arange(-3, n + 4, device=x.device)
        i = torch.where(i < 0, -i - 1, i)
        return torch.where(i >= n, 2 * n - 1 - i, i)
    t = torch.tensor([-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0], device=x.device) / 256.0
    x2 = F.conv2d(g[sym(Hc)][:, sym(Wc)][None, None], torch.outer(t, t)[None, None], stride=2)[0, 0]
    feats = []
    for img, P in ((g, 96), (x2, 48)):
        def filt(a):
            a = F.conv2d(F.pad(a[None, None], (3, 3, 0, 0), mode="replicate"), win.view(1, 1, 1, 7))
            return F.conv2d(F.pad(a, (0, 0, 3, 3), mode="replicate"), win.view(1, 1, 7, 1))[0, 0]
        mu, m2 = filt(img), filt(img * img)
        m = (img - mu) / (torch.sqrt(torch.abs(m2 - mu * mu)) + 1.0)
        k2, k1 = m.shape[0] // P, m.shape[1] // P
        mb = m.view(k2, P, k1, P).permute(0, 2, 1, 3).reshape(k2 * k1, P, P)
        cols = []
        for f, shift in enumerate((None, (0, 1), (1, 0), (1, 1), (1, -1))):
            v = mb if shift is None else mb * torch.roll(mb, shift, dims=(1, 2))
            sq, neg, pos = (v * v).double(), v < 0, v > 0
            n_neg, n_pos = neg.sum(dim=(1, 2)), pos.sum(dim=(1, 2))
            s2n, s2p = (sq * neg).sum(dim=(1, 2)), (sq * pos).sum(dim=(1, 2))
            l, r = torch.sqrt(s2n / n_neg), torch.sqrt(s2p / n_pos)
            gh = l / r
            rhat = (v.abs().double().sum(dim=(1, 2)) / (P * P)) ** 2 / ((s2n + s2p) / (P * P))
            rn = rhat * (gh ** 3 + 1.0) * (gh + 1.0) / (gh * gh + 1.0) ** 2
            ok = (n_neg > 0) & (n_pos > 0) & torch.isfinite(rn)
            j = torch.searchsorted(r_gam, torch.where(ok, rn, torch.ones_like(rn)))
            lo, hi = (j - 1).clamp(0, 9800), j.clamp(0, 9800)
            p = torch.where((r_gam[lo] - rn) ** 2 <= (r_gam[hi] - rn) ** 2, lo, hi)
            nan = torch.full_like(rn, float("nan"))
            alpha, bl, br = torch.where(ok, 0.2 + 0.001 * p, nan), torch.where(ok, l * c1[p], nan), torch.where(ok, r * c1[p], nan)
            cols += [alpha, (bl + br) / 2.0] if f == 0 else [alpha, (br - bl) * c2[p], bl, br]
        feats.append(torch.stack(cols, dim=1))
    feat = torch.cat(feats, dim=1)
    fin = torch.isfinite(feat)
    valid = fin.all(dim=1)
    rows = feat[valid]
    return torch.where(fin, feat, torch.zeros_like(feat)).sum(dim=0), fin.sum(dim=0), valid.sum(), rows.mean(dim=0), torch.cov(rows.T)


def niqe_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    grading = importlib.import_module("zero-tig_amd.grading")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)

    def dev_frame(x):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(1, 3, H, W))).to(dev)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    inputs = {"synth_lowlight": dev_frame(synth.lowlight_frame(3, H, W)), "synth_clean": dev_frame(synth.clean_frame(3, H, W)),
              "uniform_noise": dev_frame(rng.random((3, H, W), dtype=np.float32))}
    tabs = [torch.from_numpy(t).to(dev) for t in grading.niqe_tables()]
    out = {"what": "HIP-event median of %d calls at 1080 x 1920 (220 blocks, 440 tiles): block_sums = Ops.niqe_block_sums (the grey pass "
                   "over the frame, bytes = 12 H W, and the tile pass), block_sums_wgN = the same with max_workgroups = N, frame = "
                   "Ops.niqe_frame_from_sums (one workgroup), niqe = Ops.niqe_frame (all three kernels), torch = the plain-torch "
                   "composition of the same definition on the same device (tools/bench_evals_y4m.py torch_niqe), ssim_u8 = "
                   "Ops.ssim_u8_dev of the frame against the clean frame, in the same process; max_feature_gap = the largest "
                   "difference between the column means of the kernels and of the torch composition" % a.reps}
    for name, x in inputs.items():
        oi, of = torch.empty(38, dtype=torch.int64, device=dev), torch.empty(738, dtype=torch.float64, device=dev)
        one = torch.empty(1, dtype=torch.float64, device=dev)
        si, sf = ops.niqe_block_sums(x)
        row = {"block_sums": timed(lambda: ops.niqe_block_sums(x, out_i=si, out_f=sf))}
        row["block_sums"].update(bytes=12 * H * W, gbs=round(12 * H * W / row["block_sums"]["ms"] / 1e6, 1))
        for wg in (110, 220, 256):
            row["block_sums_wg%d" % wg] = timed(lambda: ops.niqe_block_sums(x, wg, out_i=si, out_f=sf))
        row["frame"] = timed(lambda: ops.niqe_frame_from_sums(si, sf, out_i=oi, out_f=of))
        row["niqe"] = timed(lambda: ops.niqe_frame(x, out_i=oi, out_f=of))
        row["torch"] = timed(lambda: torch_niqe(x, *tabs))
        row["ssim_u8"] = timed(lambda: ops.ssim_u8_dev(x, inputs["synth_clean"], out=one))
        row["torch_over_niqe"] = round(row["torch"]["ms"] / row["niqe"]["ms"], 1)
        ops.niqe_frame(x, out_i=oi, out_f=of)
        colsum, count, nv, _, _ = torch_niqe(x, *tabs)
        ints, floats = oi.tolist(), of.tolist()
        mine = np.asarray(floats[:36]) / np.maximum(np.asarray(ints[2:38]), 1)
        theirs = (colsum / count.clamp(min=1)).cpu().numpy()
        row.update(valid_blocks=ints[1], torch_valid_blocks=int(nv.item()), max_feature_gap=float(np.abs(mine - theirs).max()),
                   column_means=mine.tolist())
        out[name] = row
        print("[bench_evals_y4m] niqe %s %s" % (name, {k: v for k, v in row.items() if k != "column_means"}), file=sys.stderr, flush=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- child: the kernels of zt_flowviz.hip alone at the reduced size of --tc_scale 3 --------------------------------------
def tcviz_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    temporal = importlib.import_module("zero-tig_amd.temporal")
    y4m = importlib.import_module("zero-tig_amd.y4m")
    dev = torch.device("cuda", 0)
    weights = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in synth.make_state(3).items() if k.startswith("raft.")}
    h, w = H // 3, W // 3

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    def frame(fn, t):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(fn(t, h, w), dtype=np.float32).reshape(1, 3, h, w))).to(dev)
    cur, prev = frame(synth.lowlight_frame, 4), frame(synth.lowlight_frame, 3)
    tc = temporal.TemporalConsistency(ops, weights, dev, h, w, 1, "bf16")
    g1, g0 = frame(synth.clean_frame, 4) * 255.0, frame(synth.clean_frame, 3) * 255.0
    fb, ff = tc.flow(g1, g0), tc.flow(g0, g1)
    rad = ops.flow_radmax(fb, ff, h=h, w=w)
    pic = torch.empty((1, 3, 2 * h, 2 * w), dtype=torch.float32, device=dev)
    packed = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
    fmt = y4m.YuvFormat(2 * w, 2 * h, 420, 1, "bt709", 0)
    yuv = torch.empty(fmt.frame_bytes, dtype=torch.uint8, device=dev)
    out = {"what": "HIP-event median of %d calls at %d x %d (flows padded to %d x %d): tc_viz = zt_tc_viz_f32 of a pair (bytes: the two "
                   "frames, the two flows and the picture once each, 88 a pixel; the 20 gathered taps come on top), tc_viz_alone = "
                   "the same without a partner, radmax = zt_flow_radmax_f32 of both flows, pack = zt_flow_pack_hwc_f32, encode = "
                   "Ops.rgb_f32_to_yuv of the %d x %d picture" % (a.reps, h, w, fb.shape[2], fb.shape[3], 2 * h, 2 * w),
           "radius": rad.item()}
    for name, fn, nbytes in (("tc_viz", lambda: ops.tc_viz(cur, prev, fb, ff, rad, 4.0, out=pic), 88 * h * w),
                             ("tc_viz_alone", lambda: ops.tc_viz(cur, None, None, None, None, 4.0, out=pic), 60 * h * w),
                             ("radmax", lambda: ops.flow_radmax(fb, ff, h=h, w=w, out=rad), 16 * h * w),
                             ("pack", lambda: ops.flow_pack(fb, h, w, out=packed), 16 * h * w),
                             ("encode", lambda: ops.rgb_f32_to_yuv(pic, fmt, out=yuv), 48 * h * w + fmt.frame_bytes)):
        out[name] = dict(timed(fn), bytes=nbytes)
        out[name]["gbs"] = round(nbytes / out[name]["ms"] / 1e6, 1)
        print("[bench_evals_y4m] tcviz %s %s" % (name, out[name]), file=sys.stderr, flush=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- driver ---------------------------------------------------------------------------------------------------------------------
def _one_pair(t):
    import numpy as np
    sys.path.insert(0, ROOT)
    synth = importlib.import_module("zero-tig_amd.synth")
    y4m = importlib.import_module("zero-tig_amd.y4m")
    fmt = y4m.YuvFormat(W, H, 420, 1, "bt709", 0)
    out = []
    for fn in (synth.lowlight_frame, synth.clean_frame):
        x = np.asarray(fn(t, H, W), dtype=np.float32).reshape(3, H, W)
        out.append(y4m.encode_host((np.transpose(x, (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8), fmt))
    return out


def make_pair(tmp, frames, distinct):
    """LOW.y4m / GT.y4m: `distinct` synthetic frame pairs encoded once, written round-robin; weights from synth.make_state(3) and a
    seeded synthetic LPIPS state dict"""
    import multiprocessing as mp
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    synth = importlib.import_module("zero-tig_amd.synth")
    y4m = importlib.import_module("zero-tig_amd.y4m")
    lp = importlib.import_module("zero-tig_amd.lpips")
    with mp.get_context("spawn").Pool(min(8, distinct)) as pool:
        pairs = pool.map(_one_pair, range(distinct))
    head = y4m.Header(W, H, "30:1", "p", None, "420mpeg2", "LIMITED")
    files = {}
    for k, name in enumerate(("low", "gt")):
        files[name] = os.path.join(tmp, name + ".y4m")
        y4m.write_file(files[name], head, [pairs[i % distinct][k] for i in range(frames)])
    files["weights"] = os.path.join(tmp, "weights.pt")
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, files["weights"])
    g = torch.Generator().manual_seed(0)
    sd = {}
    for idx, (cin, cout) in zip(lp.CONV_IDX, lp.CONV_CH):
        sd["features.%d.weight" % idx] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd["features.%d.bias" % idx] = torch.randn(cout, generator=g) * 0.05
    for k, c in enumerate(lp.TAP_CH):
        sd["lin%d.model.1.weight" % k] = torch.rand(1, c, 1, 1, generator=g) / c
    files["lpips"] = os.path.join(tmp, "lpips_vgg.pt")
    torch.save(sd, files["lpips"])
    return files


def gpu_step(cmd, limit, env=None):
    """one GPU child under its own time limit; a failure ends the whole run"""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("[bench_evals_y4m] step failed with status %d, stopping: %s" % (r.returncode, " ".join(cmd)))
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=str, default="driver", choices=["driver", "kernels", "temporal", "noref", "tcviz", "color", "niqe"])
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--settings", type=str, nargs="*", default=["predict", "evals", "evals_hm", "evals_lpips", "evals_tc3", "evals_tc1"],
                    choices=["predict", "evals", "evals_hm", "evals_lpips", "evals_tc3", "evals_tc1", "evals_noref", "evals_tcviz_pic",
                             "evals_tcviz", "evals_color", "evals_niqe"])
    ap.add_argument("--skip-kernels", action="store_true", help="part (b) only")
    ap.add_argument("--skip-temporal", action="store_true", help="without the temporal kernel's own timing (part (c))")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "evals_y4m_1080p.json"))
    a = ap.parse_args()
    if a.mode == "kernels":
        return kernels_mode(a)
    if a.mode == "temporal":
        return temporal_mode(a)
    if a.mode == "noref":
        return noref_mode(a)
    if a.mode == "tcviz":
        return tcviz_mode(a)
    if a.mode == "color":
        return color_mode(a)
    if a.mode == "niqe":
        return niqe_mode(a)
    out = {"what": "evals.py --y4m_in / --y4m_gt next to predict.py --y4m_in, --graph 1 --precision bf16, over one synthetic 1080p "
                   "C420mpeg2 pair of %d frames (%d distinct), %d runs per setting, the runs alternating, one session on one box; fps "
                   "and the host-side split per frame from each script's --timing_json (predict: first frame read to last stream "
                   "closed, two Y4M streams written; evals: first frame read to the last metric read back, nothing written); "
                   "evals = --hist_match 0, no LPIPS; evals_hm = histogram matching on; evals_lpips = --hist_match 0 with a seeded "
                   "synthetic VGG state dict, --lpips_precision bf16; kernels = Ops.yuv_sse / Ops.ssim_plane alone, HIP-event median "
                   "of %d calls; evals_tc3 / evals_tc1 = evals with --tc 1 at --tc_scale 3 / 1; temporal_kernels = Ops.warp_error, "
                   "Ops.warp2 and one RAFT run of TemporalConsistency alone; evals_noref = --noref 1, no ground truth (DESIGN 8j); "
                   "noref_kernels = the two entry points of zt_noref.hip alone; evals_tcviz / evals_tcviz_pic = evals_tc3 with --tc_viz and "
                   "--tc_flo_dir / with --tc_viz alone (DESIGN 8k), tcviz_kernels = the kernels of zt_flowviz.hip alone; evals_color = "
                   "--noref 1 --color 1 (DESIGN 8m), the yardstick is evals_noref in the same run, color_kernels = zt_color_stats_f32 "
                   "alone; evals_niqe = --noref 1 --niqe MODEL (DESIGN 8n), the model fitted by tools/niqe_fit.py from every 16th frame "
                   "of the ground-truth clip, the yardstick is evals_noref in the same run, niqe_kernels = the kernels of zt_niqe.hip "
                   "alone next to a plain-torch composition" % (a.frames, a.distinct, a.repeats, a.reps),
            "cpus": len(os.sched_getaffinity(0))}
    tmp = tempfile.mkdtemp(prefix="zt_bench_evals_y4m_")
    try:
        if not a.skip_kernels:
            kj = os.path.join(tmp, "kernels.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "kernels", "--json", kj, "--reps", str(a.reps)], a.step_timeout)
            out["kernels"] = json.load(open(kj))
        if not a.skip_temporal:
            kj = os.path.join(tmp, "temporal.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "temporal", "--json", kj, "--reps", str(a.reps)], a.step_timeout)
            out["temporal_kernels"] = json.load(open(kj))
        if "evals_noref" in a.settings:
            kj = os.path.join(tmp, "noref.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "noref", "--json", kj, "--reps", str(a.reps)], a.step_timeout)
            out["noref_kernels"] = json.load(open(kj))
        if any(s.startswith("evals_tcviz") for s in a.settings):
            kj = os.path.join(tmp, "tcviz.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "tcviz", "--json", kj, "--reps", str(a.reps)], a.step_timeout)
            out["tcviz_kernels"] = json.load(open(kj))
        if "evals_color" in a.settings:
            kj = os.path.join(tmp, "color.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "color", "--json", kj, "--reps", str(a.reps)], a.step_timeout)
            out["color_kernels"] = json.load(open(kj))
        if "evals_niqe" in a.settings:
            kj = os.path.join(tmp, "niqe.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "niqe", "--json", kj, "--reps", str(a.reps)], a.step_timeout)
            out["niqe_kernels"] = json.load(open(kj))
        files = make_pair(tmp, a.frames, a.distinct)
        viz, flo = os.path.join(tmp, "viz.y4m"), os.path.join(tmp, "flo")
        env = dict(os.environ, PYTHONPATH=ROOT)
        common = ["--model_pretrain", files["weights"], "--graph", "1", "--precision", "bf16", "--y4m_in", files["low"]]
        extra = {"predict": [], "evals": ["--y4m_gt", files["gt"], "--hist_match", "0"], "evals_hm": ["--y4m_gt", files["gt"]],
                 "evals_lpips": ["--y4m_gt", files["gt"], "--hist_match", "0", "--lpips_weights", files["lpips"], "--lpips_precision", "bf16"],
                 "evals_tc3": ["--y4m_gt", files["gt"], "--hist_match", "0", "--tc", "1", "--tc_scale", "3"],
                 "evals_tc1": ["--y4m_gt", files["gt"], "--hist_match", "0", "--tc", "1", "--tc_scale", "1"],
                 "evals_noref": ["--noref", "1"]}
        extra["evals_color"] = extra["evals_noref"] + ["--color", "1"]
        if "evals_niqe" in a.settings:
            files["niqe"] = os.path.join(tmp, "niqe_model.npz")
            gpu_step([sys.executable, os.path.join(ROOT, "tools", "niqe_fit.py"), "--y4m", files["gt"], "--step", "16", "--out", files["niqe"]],
                     a.step_timeout, env=dict(os.environ, PYTHONPATH=ROOT))
            extra["evals_niqe"] = extra["evals_noref"] + ["--niqe", files["niqe"]]
        extra["evals_tcviz_pic"] = extra["evals_tc3"] + ["--tc_viz", viz]
        extra["evals_tcviz"] = extra["evals_tcviz_pic"] + ["--tc_flo_dir", flo]
        loops, wall, written = {s: [] for s in a.settings}, {s: [] for s in a.settings}, {}
        for rep in range(a.repeats):
            for s in a.settings:
                save, tj = os.path.join(tmp, "out_" + s), os.path.join(tmp, "timing_%s.json" % s)
                cmd = [sys.executable, "predict.py" if s == "predict" else "evals.py"] + common + extra[s] + ["--save", save, "--timing_json", tj]
                wall[s].append(gpu_step(cmd, a.step_timeout, env=env))
                loops[s].append(json.load(open(tj)))
                if s != "predict" and rep == 0:
                    out.setdefault("metrics", {})[s] = json.load(open(os.path.join(save, "Metrics.json")))
                    te = out["metrics"][s].get("temporal") or {}
                    if "viz" in te:                # the temporary directory's name says nothing
                        te["viz"]["path"] = os.path.basename(te["viz"]["path"])
                    if "flo_dir" in te:
                        te["flo_dir"] = os.path.basename(te["flo_dir"])
                shutil.rmtree(save, ignore_errors=True)
                if os.path.exists(viz):
                    written.setdefault(s, {}).update(viz_bytes=os.path.getsize(viz))
                    os.remove(viz)
                if os.path.isdir(flo):
                    written.setdefault(s, {}).update(flo_files=len(os.listdir(flo)))
                    shutil.rmtree(flo, ignore_errors=True)
                print("[bench_evals_y4m] %s run %d: %.1f s wall, %.2f fps" % (s, rep, wall[s][-1], loops[s][-1]["fps"]), file=sys.stderr, flush=True)
        out["end_to_end"] = {}
        for s in a.settings:
            fps = [l["fps"] for l in loops[s]]
            out["end_to_end"][s] = {"fps_runs": [round(v, 2) for v in fps], "fps_median": round(statistics.median(fps), 2),
                                    "fps_spread": round(max(fps) - min(fps), 2), "ms_per_frame_median": round(1e3 / statistics.median(fps), 3),
                                    "loop": sorted(loops[s], key=lambda l: l["fps"])[len(fps) // 2], "wall_s": [round(v, 2) for v in wall[s]]}
            if s in written:
                out["end_to_end"][s]["written"] = written[s]
        if "evals_tc3" in a.settings:
            base = out["end_to_end"]["evals_tc3"]["ms_per_frame_median"]
            for s in a.settings:
                if s.startswith("evals_tcviz"):
                    out["end_to_end"][s]["tcviz_over_tc3_ms_per_frame"] = round(out["end_to_end"][s]["ms_per_frame_median"] - base, 3)
        if "evals_noref" in a.settings and "evals_color" in a.settings:
            e2e = out["end_to_end"]
            e2e["evals_color"]["color_over_noref_ms_per_frame"] = round(e2e["evals_color"]["ms_per_frame_median"] -
                                                                        e2e["evals_noref"]["ms_per_frame_median"], 3)
        if "evals_noref" in a.settings and "evals_niqe" in a.settings:
            e2e = out["end_to_end"]
            e2e["evals_niqe"]["niqe_over_noref_ms_per_frame"] = round(e2e["evals_niqe"]["ms_per_frame_median"] -
                                                                      e2e["evals_noref"]["ms_per_frame_median"], 3)
        if "predict" in a.settings:
            base = out["end_to_end"]["predict"]["ms_per_frame_median"]
            for s in a.settings:
                out["end_to_end"][s]["ms_per_frame_over_predict"] = round(out["end_to_end"][s]["ms_per_frame_median"] - base, 3)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
