#!/usr/bin/env python3
"""Where the suggested `predict.py --y4m_scene_cut` threshold comes from.  Host only: the score is integer arithmetic
plus one division, restated here in numpy int64 (tests/test_scenecut.py pins the kernels to the same definition).

Synthetic 1080p clips of zero-tig_amd/synth.py (C420mpeg2, limited range, bt709, host encoder): per gain 12 frames, frames 0-3 of
seed 2, 4-7 of seed 7, 8-11 of seed 11, i.e. two cuts between unrelated scenes.  Prints, per gain, the largest score of a frame that
is no cut and the smallest score of a cut, then the geometric mean of the two extremes over all gains, rounded to one digit.
Usage: python tools/scene_cut_threshold.py [--size 1080x1920] [--gains 0.04 0.12 0.5] [--out FILE.json]"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (2, 7, 11)
PER_SCENE = 4


def grid(plane, yo):
    H, W = plane.shape
    gh, gw = -(-H // 16), -(-W // 16)
    v = np.zeros((gh * 16, gw * 16), dtype=np.int64)
    v[:H, :W] = np.maximum(plane.astype(np.int64) - yo, 0)
    return v.reshape(gh, 16, gw, 16).sum(axis=(1, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=str, default="1080x1920")
    ap.add_argument("--gains", type=float, nargs="+", default=[0.04, 0.12, 0.5])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    synth = importlib.import_module("zero-tig_amd.synth")
    y4m = importlib.import_module("zero-tig_amd.y4m")
    H, W = [int(v) for v in a.size.split("x")]
    fmt = y4m.YuvFormat(W, H, 420, 1, "bt709", 0)
    yo = int(fmt.decode_coef()[0])
    rows = []
    for gain in a.gains:
        prev_grid, prev_rel, no_cut, cut, mean_luma = None, 0.0, [], [], []
        for t in range(PER_SCENE * len(SEEDS)):
            f = synth.lowlight_frame(t, H, W, SEEDS[t // PER_SCENE], gain=gain)
            rgb = (np.transpose(f[0], (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
            Y = fmt.planes(y4m.encode_host(rgb, fmt))[0]
            mean_luma.append(float(Y.mean()))
            g = grid(Y, yo)
            if prev_grid is not None:
                rel = int(np.abs(g - prev_grid).sum()) / max(int((g + prev_grid).sum()), 1)
                score = min(rel, abs(rel - prev_rel))
                (cut if t % PER_SCENE == 0 else no_cut).append(score)
                prev_rel = rel
            prev_grid = g
        rows.append({"gain": gain, "mean_luma": round(sum(mean_luma) / len(mean_luma), 2), "largest_no_cut_score": max(no_cut),
                     "smallest_cut_score": min(cut), "no_cut_frames": len(no_cut), "cut_frames": len(cut)})
        print("gain %.2f: mean Y %.1f, largest no-cut score %.4f, smallest cut score %.4f" %
              (gain, rows[-1]["mean_luma"], max(no_cut), min(cut)), flush=True)
    lo, hi = max(r["largest_no_cut_score"] for r in rows), min(r["smallest_cut_score"] for r in rows)
    gm = math.sqrt(lo * hi)
    suggestion = float("%.1g" % gm)
    print("largest no-cut %.4f, smallest cut %.4f, geometric mean %.4f -> suggested threshold %g" % (lo, hi, gm, suggestion))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"size": a.size, "format": "C420mpeg2 limited bt709", "clips": rows, "largest_no_cut_score": lo,
                       "smallest_cut_score": hi, "geometric_mean": gm, "suggested_threshold": suggestion}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
