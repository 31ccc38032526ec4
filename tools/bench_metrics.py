#!/usr/bin/env python3
"""GPU box: device time of the two evals.py metrics that need real kernels, zt_ssim_u8_f32 and zt_match_histograms_f32, at
1080 x 1920 and 2160 x 3840 on a random frame (HIP events around the C ABI call with preallocated buffers, 3 warm-up calls, median
of 20), the bytes each must move and the share of the HBM peak that makes; next to them the host cost of the same two metrics
from the scipy / numpy restatement of skimage in tests/test_metrics.py (one call each).  Prints one JSON line.
Usage: python tools/bench_metrics.py [--reps 20] [--no-host]"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM_GBS = 8000.0


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    ref = None
    if not a.no_host:
        spec = importlib.util.spec_from_file_location("zt_test_metrics", os.path.join(ROOT, "tests", "test_metrics.py"))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    dev = torch.device("cuda:0")
    out = {"what": "device time of zt_ssim_u8_f32 / zt_match_histograms_f32 on a random frame, median of %d (HIP events); host = "
                   "scipy / numpy reference of tests/test_metrics.py, one call" % a.reps, "peak_hbm_gbs": PEAK_HBM_GBS, "sizes": {}}
    for H, W in ((1080, 1920), (2160, 3840)):
        rng = np.random.default_rng(H)
        src_h = rng.random((1, 3, H, W), dtype=np.float32)
        gt_h = rng.integers(0, 256, size=(1, 3, H, W)).astype(np.float32) / np.float32(255)
        src, gt = torch.from_numpy(src_h).to(dev), torch.from_numpy(gt_h).to(dev)
        n = src.numel()
        s = ops._s(src)
        npart = 3 * (-(-(H - 6) // 32)) * (-(-(W - 6) // 64))
        part = torch.empty(npart, dtype=torch.float64, device=dev)
        res = torch.empty(1, dtype=torch.float64, device=dev)
        nbytes = 8 * ((n + 3) & ~3) + 1024 * (-(-n // 4096)) + 8192
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        hm = torch.empty_like(src)
        ssim_ms, ssim_min = timed(lambda: lib.call("zt_ssim_u8_f32", src, gt, H, W, part, npart, res, s), a.reps)
        hm_ms, hm_min = timed(lambda: lib.call("zt_match_histograms_f32", src, n, gt, n, hm, scratch, nbytes, s), a.reps)
        # SSIM reads both fp32 frames once.  Matching: each of the four sort passes reads its input twice (digit counts, scatter)
        # and writes it once; the apply pass reads the source and writes the result; the template is read once.  The binary
        # search's reads of the sorted keys are served by the caches and not counted.
        ssim_bytes = 2 * 4 * n
        hm_bytes = 4 * 12 * n + 8 * n + 4 * n
        row = {"ssim_ms": round(ssim_ms, 4), "ssim_ms_min": round(ssim_min, 4), "ssim_bytes": ssim_bytes,
               "ssim_gbs": round(ssim_bytes / ssim_ms / 1e6, 1), "ssim_hbm_share": round(ssim_bytes / ssim_ms / 1e6 / PEAK_HBM_GBS, 4),
               "match_histograms_ms": round(hm_ms, 4), "match_histograms_ms_min": round(hm_min, 4), "match_histograms_bytes": hm_bytes,
               "match_histograms_gbs": round(hm_bytes / hm_ms / 1e6, 1),
               "match_histograms_hbm_share": round(hm_bytes / hm_ms / 1e6 / PEAK_HBM_GBS, 4)}
        if ref is not None:
            t0 = time.perf_counter()
            want = ref.ssim_ref(ref.u8_hwc(src_h), ref.u8_hwc(gt_h))
            row["host_ssim_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            hm_want = ref.hm_ref(src_h, gt_h)
            row["host_match_histograms_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["ssim_abs_diff_vs_host"] = abs(float(res.item()) - want)
            row["match_histograms_bit_exact_vs_host"] = bool(torch.equal(hm.cpu().view(torch.int32), torch.from_numpy(hm_want).view(torch.int32)))
        out["sizes"]["%dx%d" % (H, W)] = row
        print("[bench_metrics] %dx%d: %s" % (H, W, row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
