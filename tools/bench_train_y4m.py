#!/usr/bin/env python3
"""GPU box: what training on raw video costs next to the PNG route (train.py --y4m_in).  One MI355X, at most 16 CPUs.

(a) kernel: HIP-event median over --reps calls of `Ops.resize_planar_f32` at 2160 x 3840 -> 1080 x 1920, C = 3: the horizontal
    pass, the vertical pass and both, with the bytes each moves (source read once, result written once) and the share of the HBM peak.
(b) loop: `train.py --precision bf16 --graph 1 --epochs 4` over one synthetic 1080p clip of --frames frames (bench_predict.py's
    recipe: --distinct synthetic frames, round-robin), as
      png        the BVI-RLV PNG folder, from --parent DIR when given (a checkout of the parent commit run against this tree's
                 library), else from this tree -- the PNG route's code is the same in both
      y4m        the same pixels as one C420mpeg2 file (limited range, bt709)
      y4m_p10    the same pixels as one C420p10 file, trained at its own size
    --repeats runs per route, alternating.  Frames per second are read from the epoch log lines of epochs 1 to 3 (the loader
    workers' start-up, the first launches and the graph capture are in epoch 0); a run's figure is the median of its three epochs,
    a route's the median of its runs, and the spread is max - min over the runs.  The result pass is kept small on every route
    (a two-frame test list / --y4m_preview 2): it is not what is measured.

This driver never opens the GPU itself: every GPU step is a child process under its own `timeout -k 10`, and the first failure
ends the run.  Writes the JSON to --out and prints it as one line.
Usage: python tools/bench_train_y4m.py [--parent DIR] [--frames 256] [--out profiles/train_y4m_1080p.json]"""
import argparse
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK_HBM_GBS = 8000.0


# ---- child: the resize alone ----------------------------------------------------------------------------------------------------
def kernel_mode(a):
    import torch
    sys.path.insert(0, ROOT)
    ops = importlib.import_module("zero-tig_amd.ops").Ops(importlib.import_module("zero-tig_amd.lib").get_lib())
    C, H0, W0, H, W = 3, 2160, 3840, 1080, 1920
    x = torch.rand((1, C, H0, W0), dtype=torch.float32, device="cuda")
    tmp = torch.empty((1, C, H0, W), dtype=torch.float32, device="cuda")
    out = torch.empty((1, C, H, W), dtype=torch.float32, device="cuda")
    b_h, b_v = 4 * C * (H0 * W0 + H0 * W), 4 * C * (H0 * W + H * W)
    calls = {"horizontal": (lambda: ops.resize_planar_f32(x, (W, H0), out=tmp), b_h),
             "vertical": (lambda: ops.resize_planar_f32(tmp, (W, H), out=out), b_v),
             "both": (lambda: ops.resize_planar_f32(x, (W, H), out=out, tmp=tmp), b_h + b_v)}
    res = {"shape": "3 x 2160 x 3840 -> 3 x 1080 x 1920, fp32, clamp on", "reps": a.reps}
    for name, (fn, moved) in calls.items():
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
        res[name] = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes_moved": moved,
                     "gbs": round(moved / med / 1e6, 1), "hbm_share": round(moved / med / 1e6 / PEAK_HBM_GBS, 4)}
        print("[bench_train_y4m] resize %s %s" % (name, res[name]), file=sys.stderr, flush=True)
    with open(a.json, "w") as fh:
        json.dump(res, fh)


# ---- driver ---------------------------------------------------------------------------------------------------------------------
def epoch_fps(stdout):
    """{epoch: frames/s} from train.py's throughput lines"""
    return {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"train-epoch (\d+) throughput: .*? = ([0-9.]+) frames/s", stdout)}


def train_run(tree, extra, save, limit, lib):
    env = dict(os.environ, PYTHONPATH=tree, ZEROTIG_HIP_LIB=lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "train.py", "--precision", "bf16", "--graph", "1", "--epochs", "4", "--save", save] + extra
    r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("[bench_train_y4m] step failed with status %d, stopping: %s" % (r.returncode, " ".join(cmd)))
    fps = epoch_fps(r.stdout)
    assert sorted(fps) == [0, 1, 2, 3], fps
    return fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=str, default="driver", choices=["driver", "kernel"])
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent", type=str, default=None, help="checkout of the parent commit for the PNG route (runs against this tree's library)")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "train_y4m_1080p.json"))
    a = ap.parse_args()
    if a.mode == "kernel":
        return kernel_mode(a)
    bp = importlib.import_module("bench_predict")
    lib = os.path.join(ROOT, "zero-tig_amd", "libzerotig_hip.so")
    result = {"frames": a.frames, "distinct": a.distinct, "repeats": a.repeats, "epochs_read": [1, 2, 3],
              "png_tree": "parent" if a.parent else "this tree"}
    with tempfile.TemporaryDirectory() as tmp:
        kj = os.path.join(tmp, "kernel.json")
        bp.gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "kernel", "--json", kj, "--reps", str(a.reps)], a.step_timeout)
        result["resize"] = json.load(open(kj))
        roots, _ = bp.make_clip(tmp, a.frames, 2, a.distinct)
        open(os.path.join(roots["long"], "train_list.txt"), "w").write("S01\n")
        # the result pass walks the test list: a second scene of two frames keeps it out of the way
        d2 = os.path.join(roots["long"], "input", "S02", "low_light_10")
        os.makedirs(d2)
        for i in (1, 2):
            os.link(os.path.join(roots["long"], "input", "S01", "low_light_10", "%05d.png" % i), os.path.join(d2, "%05d.png" % i))
        open(os.path.join(roots["long"], "test_list.txt"), "w").write("S02\n")
        y8, _ = bp.make_y4m(tmp, roots, a.frames, 2, a.distinct)
        y10, _ = bp.make_y4m(tmp, roots, a.frames, 2, a.distinct, depth=10)
        routes = {"png": (a.parent or ROOT, ["--lowlight_images_path", roots["long"]]),
                  "y4m": (ROOT, ["--y4m_in", y8["long"], "--y4m_preview", "2"]),
                  "y4m_p10": (ROOT, ["--y4m_in", y10["long"], "--y4m_preview", "2"])}
        runs = {k: [] for k in routes}
        for rep in range(a.repeats):
            for name, (tree, extra) in routes.items():
                fps = train_run(tree, extra, os.path.join(tmp, "exp_%s_%d" % (name, rep)), a.step_timeout, lib)
                runs[name].append(fps)
                print("[bench_train_y4m] %s run %d: %s" % (name, rep, fps), file=sys.stderr, flush=True)
    for name, rr in runs.items():
        per_run = [statistics.median([r[e] for e in (1, 2, 3)]) for r in rr]
        result[name] = {"epoch_fps": [[r[e] for e in (0, 1, 2, 3)] for r in rr], "run_fps": per_run,
                        "fps_median": statistics.median(per_run), "fps_spread": round(max(per_run) - min(per_run), 2)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
