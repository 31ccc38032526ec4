#!/usr/bin/env python3
"""GPU box: device time of LPIPS (VGG16) at 1080 x 1920 with seeded synthetic weights (HIP events, 3 warm-up calls, median of
--reps; min next to it).  Prints one JSON line:
  ms_bf16             features of both images + distance, bf16 mode (conv1_1 / conv1_2: zt_conv2d_nhwc_bf16, the eleven wide layers:
                      zt_conv3x3_wide_bf16)
  ms_bf16_parent_path the same pass with all thirteen layers through zt_conv2d_nhwc_bf16, the only bf16 conv entry point before
                      zt_conv3x3_wide_bf16 existed (that entry point is unchanged, so this is the earlier code on the same card)
  ms_fp32             the default mode (every conv through zt_conv2d_nhwc_f32)
  layers              per conv layer of ONE image: ms on both paths, TFLOP/s and the share of the bf16 MFMA peak (2.5 PFLOP/s dense)
  ms_finetune_forward one Finetunemodel forward at 1080p (the enhancement that LPIPS grades), for scale
Usage: python tools/bench_lpips.py [--reps 10] [--no-fp32]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BF16_TFLOPS = 2500.0


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


def synthetic_weights(lp, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, (cin, cout) in zip(lp.CONV_IDX, lp.CONV_CH):
        sd["features.%d.weight" % idx] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd["features.%d.bias" % idx] = torch.randn(cout, generator=g) * 0.05
    for k, c in enumerate(lp.TAP_CH):
        sd["lin%d.model.1.weight" % k] = torch.rand(1, c, 1, 1, generator=g) / c
    return sd


class ParentPathOps:
    """Ops whose wide-layer call goes to zt_conv2d_nhwc_bf16 (tiled kernel, 32 couts per workgroup), as before this kernel existed."""

    def __init__(self, ops):
        self._ops = ops

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def conv3x3_wide_bf16(self, x, wdev, bias, Cout, relu=True, out=None):
        return self._ops.conv2d_bf16(x, wdev, bias, Cout, 3, 3, pad=(1, 1), act="relu" if relu else None, out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-fp32", action="store_true")
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920))
    a = ap.parse_args()
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()
    ops_mod = importlib.import_module("zero-tig_amd.ops")
    lp = importlib.import_module("zero-tig_amd.lpips")
    synth = importlib.import_module("zero-tig_amd.synth")
    ops, CV = ops_mod.Ops(lib), ops_mod.CV
    dev = torch.device("cuda:0")
    H, W = a.size
    sd = synthetic_weights(lp)
    img = torch.from_numpy(np.clip(synth.lowlight_frame(0, H, W) * np.float32(3), 1e-4, 1).astype(np.float32)).to(dev)
    gt = torch.from_numpy(np.asarray(synth.clean_frame(0, H, W), dtype=np.float32).reshape(1, 3, H, W)).to(dev)
    out = {"what": "LPIPS (VGG16, synthetic weights) of one %d x %d image pair, median of %d (HIP events)" % (H, W, a.reps),
           "peak_bf16_tflops": PEAK_BF16_TFLOPS}

    m_new = lp.LpipsVGG(ops, sd, dev, "bf16")
    m_old = lp.LpipsVGG(ParentPathOps(ops), sd, dev, "bf16")
    out["lpips_bf16"], out["lpips_bf16_parent_path"] = m_new(img, gt), m_old(img, gt)
    out["ms_bf16"], out["ms_bf16_min"] = [round(v, 3) for v in timed(lambda: m_new(img, gt), a.reps)]
    out["ms_bf16_parent_path"], out["ms_bf16_parent_path_min"] = [round(v, 3) for v in timed(lambda: m_old(img, gt), a.reps)]
    print("[bench_lpips] pair: new %.3f ms, parent path %.3f ms" % (out["ms_bf16"], out["ms_bf16_parent_path"]), file=sys.stderr, flush=True)

    layers, h, w = [], H, W
    g = torch.Generator().manual_seed(1)
    for idx, (wdev, bias, cin, cout) in zip(lp.CONV_IDX, m_new.layers):
        if idx in lp.POOL_BEFORE:
            h, w = h // 2, w // 2
        ld = max(cin, 8)
        x = CV((torch.rand(1, h, w, ld, generator=g) * (1.0 if cin > 3 else 0.0)).bfloat16().to(dev), 0, cin)
        if cin == 3:
            x.t[..., :3] = torch.randn(1, h, w, 3, generator=g).bfloat16().to(dev)
        y = torch.empty((1, h, w, cout), dtype=torch.bfloat16, device=dev)
        parent = lambda: ops.conv2d_bf16(x, wdev, bias, cout, 3, 3, pad=(1, 1), act="relu", out=y)
        wide = cin >= 64 and cout >= 128
        new = (lambda: ops.conv3x3_wide_bf16(x, wdev, bias, cout, relu=True, out=y)) if wide else parent
        ms_new, _ = timed(new, a.reps)
        ms_par, _ = timed(parent, a.reps) if wide else (ms_new, ms_new)
        flop = 2.0 * 9 * cin * cout * h * w
        row = {"features_idx": idx, "cin": cin, "cout": cout, "h": h, "w": w, "kernel": "wide" if wide else "zt_conv2d_nhwc_bf16",
               "ms": round(ms_new, 4), "ms_parent_path": round(ms_par, 4), "tflops": round(flop / ms_new / 1e9, 1),
               "peak_share": round(flop / ms_new / 1e9 / PEAK_BF16_TFLOPS, 4)}
        layers.append(row)
        print("[bench_lpips] %s" % row, file=sys.stderr, flush=True)
    out["layers"] = layers
    wide_rows = [r for r in layers if r["kernel"] == "wide"]
    out["ms_wide_layers"] = round(sum(r["ms"] for r in wide_rows), 3)
    out["ms_wide_layers_parent_path"] = round(sum(r["ms_parent_path"] for r in wide_rows), 3)
    flop_wide = sum(2.0 * 9 * r["cin"] * r["cout"] * r["h"] * r["w"] for r in wide_rows)
    out["wide_layers_tflops"] = round(flop_wide / out["ms_wide_layers"] / 1e9, 1)
    out["wide_layers_peak_share"] = round(flop_wide / out["ms_wide_layers"] / 1e9 / PEAK_BF16_TFLOPS, 4)

    if not a.no_fp32:
        m32 = lp.LpipsVGG(ops, sd, dev, "fp32")
        out["lpips_fp32"] = m32(img, gt)
        out["ms_fp32"], out["ms_fp32_min"] = [round(v, 3) for v in timed(lambda: m32(img, gt), max(2, a.reps // 3), warmup=1)]
        del m32
        torch.cuda.empty_cache()

    sys.path.insert(0, ROOT)
    model_mod = importlib.import_module("model.model")
    with tempfile.TemporaryDirectory() as td:
        wp = os.path.join(td, "weights.pt")
        torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, wp)
        torch.manual_seed(2)
        net = model_mod.Finetunemodel(argparse.Namespace(dataset="RLV", of_scale=3, model_pretrain=wp)).to(dev)
        net.eval()
        net.is_new_seq = True
        with torch.no_grad():
            net(img)
            net.is_new_seq = False
            out["ms_finetune_forward"], out["ms_finetune_forward_min"] = [round(v, 3) for v in timed(lambda: net(img), a.reps)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
