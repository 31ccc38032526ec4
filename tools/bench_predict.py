#!/usr/bin/env python3
"""GPU box: what the device PNG encoder (zt_png.hip, `--device_png 1` / `2`) buys predict.py.  One MI355X, at most 16 CPUs.

(a) encode cost: HIP-event median over --reps calls of `Ops.png_encode` alone at 1080p and 4K, mode 1 and mode 2 in the same
    process, on the "enhanced_noisy" synthetic frame (low-light frame 3 of zero-tig_amd/synth.py scaled to mean 0.4 plus sigma-4
    noise) and on its letterboxed form (the top and bottom 138 / 1080 of the rows black): the stream size, and the share of the
    HBM peak for the bytes the encode touches (input once, filtered scanlines written once and read twice -- three times in mode 2,
    which walks them once more for the run histogram --, the stream zeroed, packed, read and gathered).
(b) end to end: predict.py --graph 1 --precision bf16 over --frames synthetic 1080p PNG inputs in a temporary directory, for
      parent         a checkout of the parent commit (--parent DIR; skipped when not given), run against this tree's library
      device_png_0   this tree, PIL on the loop's thread
      device_png_1   this tree, device encoder + threaded writer
      device_png_2   the same with the encoder's mode 2 (run-length matches)
    Frames per second from the first frame read to the last file closed (predict.py --timing_json, with the host-side split per
    frame: decode wait, step, copy wait, writer wait) for each of --repeats runs over the --frames inputs, their median and their
    spread (max - min), and -- the only figure a tree without --timing_json can give -- the differential rate
    (frames - short) / (median wall(frames) - wall(short)) of whole-process runs, which cancels the start-up.

(c) --y4m: raw video instead of PNG files (predict.py --y4m_in / zt_yuv.hip).  The clip's frames, converted by the host encoder of
    zero-tig_amd/y4m.py (C420mpeg2, limited range, bt709), form one Y4M file; `y4m` in "end_to_end" is predict.py --graph 1
    --precision bf16 --y4m_in over it (two Y4M streams written), measured like the PNG settings, and "convert" holds the three
    conversions alone at 1080p: HIP-event median over --reps calls, the bytes each moves and the share of the HBM peak.
    --y4m-depth B (9 .. 16): the same loop over the clip as C420pB as "y4m_pB", its runs alternating with those of "y4m", and the
    two deep conversions (zt_yuv.hip) next to the 8-bit ones in "convert".
    --scene-cut T [T ..]: the same loop with predict.py --y4m_scene_cut T as "y4m_scene_cut_T", its runs alternating with those of
    "y4m" (flag off), with the time the loop was blocked for the detector (scene_wait_ms) and the sequences restarted (cuts); "scene"
    holds the two kernels of zt_scene.hip alone.

This driver never opens the GPU itself: every GPU step is a child process under its own `timeout -k 10`, and the first failure
ends the run.  Writes the JSON to --out and prints it as one line.
Usage: python tools/bench_predict.py [--parent DIR] [--frames 64] [--short 16] [--out profiles/predict_png_1080p.json]
       python tools/bench_predict.py --skip-encode --frames 256 --short 64 --settings 1 2 --out profiles/predict_png_1080p_256.json
       python tools/bench_predict.py --skip-encode --y4m --frames 256 --short 64 --settings 1 --out profiles/predict_y4m_1080p.json
       python tools/bench_predict.py --skip-encode --y4m --scene-cut 0.5 0.03 --frames 256 --short 64 --settings \
                                     --out profiles/predict_y4m_scene_cut_1080p.json
       python tools/bench_predict.py --skip-encode --y4m --y4m-depth 10 --frames 256 --short 64 --settings \
                                     --out profiles/predict_y4m_deep_1080p.json"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_HBM_GBS = 8000.0


# ---- child: the encode alone ----------------------------------------------------------------------------------------------------
def encode_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    out = {}
    for size in a.sizes:
        H, W = [int(v) for v in size.split("x")]
        f = synth.lowlight_frame(3, H, W)[0].transpose(1, 2, 0).astype(np.float64)
        e = np.clip(f * (0.4 / f.mean()), 0, 1)
        noisy = np.clip(np.round(e * 255 + np.random.default_rng(4).normal(0, 4, e.shape)), 0, 255).astype(np.uint8)
        box = noisy.copy()
        bar = H * 138 // 1080
        box[:bar] = 0
        box[H - bar:] = 0
        ws_bytes, cap = ops.png_sizes(H, W)
        stream = torch.empty(cap, dtype=torch.uint8, device="cuda")
        out[size] = {"workspace_bytes": ws_bytes, "capacity_bytes": cap, "raw_bytes": 3 * H * W}
        for fname, arr in (("enhanced_noisy", noisy), ("letterbox", box)):
            u8 = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
            row = {}
            for mode in (1, 2):
                for _ in range(3):
                    _, n = ops.png_encode(u8, out=stream, mode=mode)
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ops.png_encode(u8, out=stream, mode=mode)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                nbytes = int(n.item())
                scan = H * (3 * W + 1)
                touched = 3 * H * W + (2 + mode) * scan + 4 * nbytes
                med = statistics.median(ms)
                row["mode_%d" % mode] = {"encode_ms": round(med, 4), "encode_ms_min": round(min(ms), 4), "stream_bytes": nbytes,
                                         "bytes_touched": touched, "gbs": round(touched / med / 1e6, 1),
                                         "hbm_share": round(touched / med / 1e6 / PEAK_HBM_GBS, 4)}
            row["mode_2_over_mode_1_ms"] = round(row["mode_2"]["encode_ms"] / row["mode_1"]["encode_ms"], 3)
            out[size][fname] = row
            print("[bench_predict] encode %s %s %s" % (size, fname, row), file=sys.stderr, flush=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- child: the colour conversions alone -------------------------------------------------------------------------------------------
def convert_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    y4m = importlib.import_module("zero-tig_amd.y4m")
    H, W = 1080, 1920
    fmt = y4m.YuvFormat(W, H, 420, 1, "bt709", 0)
    rgb = (np.transpose(synth.lowlight_frame(3, H, W)[0], (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
    payload = torch.from_numpy(y4m.encode_host(rgb, fmt)).cuda()
    x = torch.empty((1, 3, H, W), dtype=torch.float32, device="cuda")
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    back = torch.empty_like(payload)
    calls = {"yuv_to_rgb_u8": (lambda: ops.yuv_to_rgb_u8(payload, fmt, out=u8), fmt.frame_bytes + 3 * H * W),
             "yuv_to_planar_f32": (lambda: ops.yuv_to_planar_f32(payload, fmt, out=x), fmt.frame_bytes + 12 * H * W),
             "rgb_f32_to_yuv": (lambda: ops.rgb_f32_to_yuv(x, fmt, out=back), fmt.frame_bytes + 12 * H * W)}
    out = {"format": "1080x1920 C420mpeg2 limited bt709", "payload_bytes": fmt.frame_bytes}
    if a.y4m_depth > 8:                             # the two deep conversions next to the 8-bit ones, same frame, same session
        deep = fmt._replace(depth=a.y4m_depth)
        payload16 = torch.from_numpy(y4m.encode_host(rgb.astype(np.uint16) * 257, deep)).cuda()
        back16 = torch.empty_like(payload16)
        calls["yuv16_to_planar_f32"] = (lambda: ops.yuv_to_planar_f32(payload16, deep, out=x), deep.frame_bytes + 12 * H * W)
        calls["rgb_f32_to_yuv16"] = (lambda: ops.rgb_f32_to_yuv(x, deep, out=back16), deep.frame_bytes + 12 * H * W)
        out["deep_format"] = "1080x1920 C420p%d limited bt709" % a.y4m_depth
        out["deep_payload_bytes"] = deep.frame_bytes
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
        out[name] = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes_moved": moved,
                     "gbs": round(moved / med / 1e6, 1), "hbm_share": round(moved / med / 1e6 / PEAK_HBM_GBS, 4)}
        print("[bench_predict] convert %s %s" % (name, out[name]), file=sys.stderr, flush=True)
    with open(a.json, "w") as fh:
        json.dump(out, fh)


# ---- child: the scene-cut kernels alone -----------------------------------------------------------------------------------------------
def scene_mode(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    y4m = importlib.import_module("zero-tig_amd.y4m")
    H, W = 1080, 1920
    fmt = y4m.YuvFormat(W, H, 420, 1, "bt709", 0)
    pay = []
    for t in (3, 4):
        rgb = (np.transpose(synth.lowlight_frame(t, H, W)[0], (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
        pay.append(torch.from_numpy(y4m.encode_host(rgb, fmt)).cuda())
    shifted = torch.empty(H * W + 1, dtype=torch.uint8, device="cuda")[1:]      # one byte off a 16-byte boundary: the byte path
    shifted.copy_(pay[0][:H * W])
    cells = ((H + 15) // 16) * ((W + 15) // 16)
    g = [torch.empty(cells, dtype=torch.int32, device="cuda") for _ in range(3)]
    pair = torch.empty(2, dtype=torch.int64, device="cuda")
    ops.luma_grid(pay[1], fmt, out=g[1])
    calls = {"luma_grid_16_byte_loads": (lambda: ops.luma_grid(pay[0], fmt, out=g[0]), H * W + 4 * cells),
             "luma_grid_byte_loads": (lambda: ops.luma_grid(shifted, fmt, out=g[2]), H * W + 4 * cells),
             "grid_sad": (lambda: ops.grid_sad(g[0], g[1], out=pair), 8 * cells + 16)}
    out = {"format": "1080x1920 luma plane, 68 x 120 cells", "cells": cells}
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
        out[name] = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes_moved": moved,
                     "gbs": round(moved / med / 1e6, 1)}
        print("[bench_predict] scene %s %s" % (name, out[name]), file=sys.stderr, flush=True)
    assert torch.equal(g[0], g[2]), "the byte path and the 16-byte path disagree"
    sad, tot = pair.tolist()
    out["pair_of_frames_3_4"] = {"sad": sad, "tot": tot, "rel": sad / max(tot, 1)}
    with open(a.json, "w") as fh:
        json.dump(out, fh)


def make_y4m(tmp, roots, frames, short, distinct, depth=8):
    """the PNG clip's pixels as Y4M files (host encoder; the `distinct` frames encoded once, written round-robin); depth > 8: as
    C420pN, from the same pixels as 16-bit levels (x 257)"""
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    y4m = importlib.import_module("zero-tig_amd.y4m")
    head = y4m.Header(1920, 1080, "30:1", "p", None, "420mpeg2" if depth == 8 else "420p%d" % depth, "LIMITED")
    fmt = head.format("bt709")
    d = os.path.join(roots["long"], "input", "S01", "low_light_10")
    rgb = [np.asarray(Image.open(os.path.join(d, "%05d.png" % (i + 1)))) for i in range(min(distinct, frames))]
    pay = [y4m.encode_host(p if depth == 8 else p.astype(np.uint16) * 257, fmt) for p in rgb]
    files = {}
    for name, n in (("long", frames), ("short", short)):
        files[name] = os.path.join(tmp, "clip%s_%s.y4m" % ("" if depth == 8 else "_p%d" % depth, name))
        y4m.write_file(files[name], head, [pay[i % len(pay)] for i in range(n)])
    return files, fmt.frame_bytes


# ---- driver ---------------------------------------------------------------------------------------------------------------------
def _one_frame(args):
    import numpy as np
    from PIL import Image
    sys.path.insert(0, ROOT)
    synth = importlib.import_module("zero-tig_amd.synth")
    t, path = args
    a = synth.lowlight_frame(t, 1080, 1920)
    Image.fromarray((np.transpose(a[0], (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)).save(path, compress_level=1)
    return path


def make_clip(tmp, frames, short, distinct):
    """RLV-layout inputs: `distinct` different synthetic frames written once and copied round-robin to `frames` consecutive names
    (and the first `short` of them to a second tree); weights from synth.make_state(3)"""
    import multiprocessing as mp
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    synth = importlib.import_module("zero-tig_amd.synth")
    src = os.path.join(tmp, "distinct")
    os.makedirs(src)
    with mp.get_context("spawn").Pool(min(8, distinct)) as pool:
        files = pool.map(_one_frame, [(t, os.path.join(src, "%d.png" % t)) for t in range(distinct)])
    roots = {}
    for name, n in (("long", frames), ("short", short)):
        d = os.path.join(tmp, name, "RLV", "input", "S01", "low_light_10")
        os.makedirs(d)
        for i in range(n):
            shutil.copyfile(files[i % distinct], os.path.join(d, "%05d.png" % (i + 1)))
        open(os.path.join(tmp, name, "RLV", "test_list.txt"), "w").write("S01\n")
        roots[name] = os.path.join(tmp, name, "RLV")
    weights = os.path.join(tmp, "weights.pt")
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, weights)
    return roots, weights


def gpu_step(cmd, limit, env=None, cwd=ROOT):
    """one GPU child under its own time limit; a failure ends the whole run"""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, env=env, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("[bench_predict] step failed with status %d, stopping: %s" % (r.returncode, " ".join(cmd)))
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=str, default="driver", choices=["driver", "encode", "convert", "scene"])
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--sizes", type=str, nargs="+", default=["1080x1920", "2160x3840"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent", type=str, default=None, help="checkout of the parent commit (runs against this tree's library)")
    ap.add_argument("--y4m-depth", type=int, default=8, choices=[8, 9, 10, 12, 14, 16],
                    help="with --y4m, B > 8: also the Y4M loop over the same clip as C420pB (setting y4m_pB, its runs alternating with "
                         "those of y4m), and the two deep conversions in convert")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--short", type=int, default=16)
    ap.add_argument("--settings", type=int, nargs="*", default=[0, 1, 2], choices=[0, 1, 2],
                    help="the --device_png values of part (b); a longer clip (--frames 256 --short 64 --settings 1 2) narrows the spread; "
                         "none: the PNG loop is not run")
    ap.add_argument("--skip-encode", action="store_true", help="part (b) only")
    ap.add_argument("--short-repeats", type=int, default=1,
                    help="runs over the --short inputs per setting; the differential rate uses their median (one run leaves it noisy)")
    ap.add_argument("--y4m", action="store_true", help="part (c): the Y4M loop next to the PNG settings, and the conversions alone")
    ap.add_argument("--scene-cut", type=float, nargs="+", default=[],
                    help="with --y4m: also the Y4M loop with predict.py --y4m_scene_cut T for each T given (settings y4m_scene_cut_T, next "
                         "to y4m = flag off, the runs alternating), their loop.scene_wait_ms and loop.cuts, and scene = the two kernels "
                         "of zt_scene.hip alone at 1080p.  The clip repeats --distinct frames, and the jump back to the first one scores "
                         "0.054: a T above that measures the detector alone, a T below it also a restarted sequence every --distinct frames")
    ap.add_argument("--repeats", type=int, default=3, help="runs over the --frames inputs per setting (the spread between them is reported)")
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "predict_png_1080p.json"))
    a = ap.parse_args()
    if a.mode == "encode":
        return encode_mode(a)
    if a.mode == "convert":
        return convert_mode(a)
    if a.mode == "scene":
        return scene_mode(a)
    out = {"what": "predict.py --graph 1 --precision bf16 over %d synthetic 1080p PNG inputs (%d distinct): frames per second from the "
                   "first frame read to the last file closed (timing_json), the differential whole-process rate over %d and %d "
                   "frames, and the host-side split per frame, %d runs per setting; encode = Ops.png_encode alone, mode 1 and 2, "
                   "HIP-event median of %d calls" % (a.frames, a.distinct, a.frames, a.short, a.repeats, a.reps),
           "cpus": len(os.sched_getaffinity(0)), "peak_hbm_gbs": PEAK_HBM_GBS}
    out["what"] += ("; loop.decode_wait_ms includes the wait for the FIRST frame (loader start-up), which `seconds` / `fps` exclude: "
                    "loop.decode_wait_steady_ms_max = (seconds - frames * (step + copy_wait + write + writer_wait)) / (frames - 1) "
                    "bounds the wait per frame after the first; differential_fps from the medians of %d short and %d long runs"
                    % (a.short_repeats, a.repeats))
    if a.y4m:
        out["what"] += ("; y4m = the same loop over the clip's pixels as one Y4M file (C420mpeg2, limited, bt709; host encoder), "
                        "predict.py --y4m_in, two Y4M streams written; its loop.writer_thread_event_ms / writer_thread_io_ms = the "
                        "two writer threads' time per frame waiting for the step's event / inside write(); convert = "
                        "Ops.yuv_to_rgb_u8, yuv_to_planar_f32, rgb_f32_to_yuv alone at 1080p, HIP-event median of %d calls" % a.reps)
    tmp = tempfile.mkdtemp(prefix="zt_bench_predict_")
    try:
        if not a.skip_encode:
            ej = os.path.join(tmp, "encode.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "encode", "--json", ej, "--reps", str(a.reps), "--sizes"]
                     + a.sizes, a.step_timeout)
            out["encode"] = json.load(open(ej))
        if a.y4m:
            cj = os.path.join(tmp, "convert.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "convert", "--json", cj, "--reps", str(a.reps), "--y4m-depth",
                      str(a.y4m_depth)], a.step_timeout)
            out["convert"] = json.load(open(cj))
        if a.y4m and a.scene_cut:
            sj = os.path.join(tmp, "scene.json")
            gpu_step([sys.executable, os.path.abspath(__file__), "--mode", "scene", "--json", sj, "--reps", str(a.reps)], a.step_timeout)
            out["scene"] = json.load(open(sj))
            out["what"] += ("; y4m_scene_cut_T = the y4m loop with --y4m_scene_cut T (loop.scene_wait_ms = the time pop() was blocked, part "
                            "of step_ms; loop.cuts = sequences restarted), its runs alternating with those of y4m; scene = "
                            "Ops.luma_grid (16-byte and byte loads) and Ops.grid_sad alone, HIP-event median of %d calls" % a.reps)
        roots, weights = make_clip(tmp, a.frames, a.short, a.distinct)
        y4m_files = make_y4m(tmp, roots, a.frames, a.short, a.distinct)[0] if a.y4m else None
        deep_name = "y4m_p%d" % a.y4m_depth
        deep_files = make_y4m(tmp, roots, a.frames, a.short, a.distinct, a.y4m_depth)[0] if a.y4m and a.y4m_depth > 8 else None
        so = os.path.join(ROOT, "zero-tig_amd", "libzerotig_hip.so")
        configs = ([("parent", a.parent, [])] if a.parent else []) + [("device_png_%d" % v, ROOT, ["--device_png", str(v)])
                                                                      for v in a.settings]
        if a.y4m:
            configs.append(("y4m", ROOT, ["--y4m_in"]))
            if deep_files:
                configs.append((deep_name, ROOT, ["--y4m_in"]))
                out["what"] += ("; %s = the y4m loop over the same pixels as C420p%d (16-bit levels = 257 x the PNG's), streams written at "
                                "that depth, its runs alternating with those of y4m; convert.yuv16_to_planar_f32 / rgb_f32_to_yuv16 = "
                                "the deep conversions" % (deep_name, a.y4m_depth))
            for T in a.scene_cut:
                configs.append(("y4m_scene_cut_%g" % T, ROOT, ["--y4m_scene_cut", str(T), "--y4m_in"]))
        out["end_to_end"] = {}
        state = {name: ({}, {"short": [], "long": []}, []) for name, _, _ in configs}

        def run_once(name, tree, extra, which, n):
            row, wall, loops = state[name]
            is_y4m = name.startswith("y4m")
            env = dict(os.environ, PYTHONPATH=tree, ZEROTIG_HIP_LIB=so)
            save = os.path.join(tmp, "out_%s_%s" % (name, which))
            cmd = [sys.executable, "predict.py", "--dataset", "RLV", "--lowlight_images_path", roots[which], "--model_pretrain",
                   weights, "--save", save, "--graph", "1", "--precision", "bf16"] + extra
            if is_y4m:
                cmd.append((deep_files if name == deep_name else y4m_files)[which])
            tj = os.path.join(tmp, "timing_%s_%s.json" % (name, which))
            if extra:
                cmd += ["--timing_json", tj]
            wall[which].append(gpu_step(cmd, a.step_timeout, env=env, cwd=tree))
            written = sum(len(fs) for _, _, fs in os.walk(save))
            assert written == (2 if is_y4m else 2 * n), (name, which, written)
            if which == "long":
                row["output_bytes_per_frame"] = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(save) for f in fs) // n
                if extra:
                    loops.append(json.load(open(tj)))
            shutil.rmtree(save)
            print("[bench_predict] %s %s %.1f s" % (name, which, wall[which][-1]), file=sys.stderr, flush=True)

        # the runs of y4m and y4m_scene_cut alternate (same minutes, same neighbours on the box); every other setting runs on its own
        groups = [[c] for c in configs if not c[0].startswith("y4m")] + ([[c for c in configs if c[0].startswith("y4m")]] if a.y4m else [])
        for group in groups:
            for which, n, times in (("short", a.short, a.short_repeats), ("long", a.frames, a.repeats)):
                for _ in range(times):
                    for name, tree, extra in group:
                        run_once(name, tree, extra, which, n)
        for name, tree, extra in configs:
            row, wall, loops = state[name]
            if loops:
                fps = [l["fps"] for l in loops]
                row["loop"] = sorted(loops, key=lambda l: l["fps"])[len(loops) // 2]          # the median run's split
                lp = row["loop"]
                busy = sum(lp.get(k, 0.0) for k in ("step_ms", "copy_wait_ms", "write_ms", "writer_wait_ms"))
                if lp["frames"] > 1:
                    lp["decode_wait_steady_ms_max"] = max(0.0, (1e3 * lp["seconds"] - lp["frames"] * busy) / (lp["frames"] - 1))
                row["fps_runs"] = [round(v, 2) for v in fps]
                row["fps_median"] = round(statistics.median(fps), 2)
                row["fps_spread"] = round(max(fps) - min(fps), 2)
                if "scene_wait_ms" in lp:
                    row["scene_wait_ms_runs"] = [round(l["scene_wait_ms"], 4) for l in loops]
                    row["cuts_runs"] = [l["cuts"] for l in loops]
            row["wall_s"] = {k: [round(v, 2) for v in vs] for k, vs in wall.items()}
            row["differential_fps"] = round((a.frames - a.short) / (statistics.median(wall["long"]) - statistics.median(wall["short"])), 2)
            out["end_to_end"][name] = row
            print("[bench_predict] %s %s" % (name, row), file=sys.stderr, flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
