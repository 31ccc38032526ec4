#!/usr/bin/env python3
"""GPU box: inference time per frame of the synthetic clip (zero-tig_amd/synth.py), steady-state frames (RAFT + warp included),
by HIP events around every frame, median of --frames timed frames after --warmup frames of every shape and mode.

Per frame size (540p, 1080p, 4K) and precision (fp32, bf16) it reports ms per frame of
  eager        the eager `Finetunemodel.forward` (the API of the reference; weights repacked per frame, BatchNorm as its own passes)
  stream       `InferStep(use_graph=False)`: the streaming plan, launched eagerly
  graph        `InferStep(use_graph=True)`: the same plan as one hipGraph replay
and the kernel launches per steady-state frame of the first two.  Per Denoise call (Denoise_1 and Denoise_2 shapes, bf16) it times
the one-launch kernel zt_denoise_fused_bf16 against the pack + three convolutions + tail chain, alternated in the same process (ten
calls per hipGraph replay, so no host launch time on either side):
`Engine.FUSED_DENOISE_MIN_PIXELS` is set from this A/B.

Needs the MI355X (no fallback).  Writes the JSON to --out and prints it as one line.
Usage: python tools/bench_infer.py [--frames 50] [--warmup 5] [--sizes 540x960 1080x1920 2160x3840] [--out profiles/infer_540p_1080p_4k.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_frame_ms(fn, xs, frames, warmup):
    """fn(frame index) once per frame; -> (median, min) of the timed frames"""
    for t in range(warmup):
        fn(t)
    torch.cuda.synchronize()
    ms = []
    for t in range(frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warmup + t)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    return round(statistics.median(ms), 4), round(min(ms), 4)


def launches(lib, fn):
    before = dict(lib.calls)
    fn()
    return sum(v - before.get(k, 0) for k, v in lib.calls.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=str, nargs="+", default=["540x960", "1080x1920", "2160x3840"])
    ap.add_argument("--precisions", type=str, nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--ab-reps", type=int, default=30)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "infer_540p_1080p_4k.json"))
    a = ap.parse_args()
    lib = importlib.import_module("zero-tig_amd.lib").get_lib()               # raises without a HIP device
    ops = importlib.import_module("zero-tig_amd.ops").Ops(lib)
    synth = importlib.import_module("zero-tig_amd.synth")
    net_mod = importlib.import_module("zero-tig_amd.network")
    infer = importlib.import_module("zero-tig_amd.infer")
    dev = torch.device("cuda:0")
    state = {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}
    out = {"what": "ms per steady-state frame (HIP events, median of %d after %d warm-up frames; min next to it)" % (a.frames, a.warmup),
           "device": torch.cuda.get_device_name(0), "of_scale": 3, "sizes": {}, "denoise_ab": []}

    def model(precision):
        net = net_mod.Finetunemodel(argparse.Namespace(dataset="RLV", of_scale=3), ops=ops, precision=precision)
        net.load_state_dict(state)
        net = net.to(dev)
        net.eval()
        return net

    for size in a.sizes:
        H, W = [int(v) for v in size.split("x")]
        xs = [torch.from_numpy(synth.lowlight_frame(t, H, W, 2)).to(dev) for t in range(4)]
        rows = {}
        for precision in a.precisions:
            row = {}
            net = model(precision)

            def eager(t, net=net):
                net.is_new_seq = t == 0
                with torch.no_grad():
                    return net(xs[t % 4])
            row["eager_ms"], row["eager_ms_min"] = per_frame_ms(eager, xs, a.frames, a.warmup)
            row["eager_launches"] = launches(lib, lambda: eager(1))
            del net
            for key, use_graph in (("stream", False), ("graph", True)):
                step = infer.InferStep(model(precision), use_graph=use_graph)
                fn = lambda t, step=step: step(xs[t % 4], is_new_seq=(t == 0))
                row[key + "_ms"], row[key + "_ms_min"] = per_frame_ms(fn, xs, a.frames, a.warmup)
                if not use_graph:
                    row["stream_launches"] = launches(lib, lambda: fn(1))
                else:
                    assert step.n_captures == 1
                del step
            torch.cuda.empty_cache()
            rows[precision] = row
            print("[bench_infer] %s %s %s" % (size, precision, row), file=sys.stderr, flush=True)
        out["sizes"][size] = rows

        # ---- one Denoise call: fused launch against the chain, alternated
        net = model("bf16")
        eng, _ = net._plan()
        with torch.no_grad():
            wp = eng.prepare_stream()
        g = torch.Generator().manual_seed(0)
        pl = [torch.rand(1, 3, H, W, generator=g).to(dev) for _ in range(4)]
        for name, pre, srcs, refs, cin, cout in (("D1", "denoise_1", [pl[0]], [pl[0]], 3, 3), ("D2", "denoise_2", pl, [pl[2], pl[3]], 12, 6)):
            def call(fused):
                return eng._denoise_stream(pre, srcs, refs, wp, H, W, cin, cout, fused=fused)
            n_launch = {f: launches(lib, lambda f=f: call(f)) for f in (True, False)}
            for _ in range(3):
                call(True), call(False)
            torch.cuda.synchronize()
            # ten calls per hipGraph, so that neither side pays host launch time (the streaming plan is replayed as a graph)
            graphs = {}
            for mp in (True, False):
                gr = torch.cuda.CUDAGraph()
                with torch.no_grad(), torch.cuda.graph(gr, capture_error_mode="thread_local"):
                    keep = [call(mp) for _ in range(10)]
                graphs[mp] = (gr, keep)
                gr.replay()
            torch.cuda.synchronize()
            ms = {True: [], False: []}
            for _ in range(a.ab_reps):
                for mp in (True, False):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    graphs[mp][0].replay()
                    e1.record()
                    e1.synchronize()
                    ms[mp].append(e0.elapsed_time(e1) / 10.0)
            del graphs
            d = float((call(True) - call(False)).abs().max())
            row = {"size": size, "call": name, "fused_us": round(1e3 * statistics.median(ms[True]), 1),
                   "chain_us": round(1e3 * statistics.median(ms[False]), 1), "fused_launches": n_launch[True],
                   "chain_launches": n_launch[False], "max_abs_diff": d}
            out["denoise_ab"].append(row)
            print("[bench_infer] %s" % row, file=sys.stderr, flush=True)
        del net, eng, wp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
