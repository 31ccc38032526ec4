#!/usr/bin/env python3
"""Fit the pristine model of `evals.py --niqe` from well-lit footage of your own (Mittal, Soundararajan and Bovik 2013,
section 3).  Every `--step`-th frame of the clip is decoded on the device (the reader and the colour conversion of predict.py
--y4m_in) and passed to `Ops.niqe_block_sums`; the block selection (sharpness above 0.75 of the frame's sharpest block), the fits
and the accumulation run in numpy float64 on the host (`grading.NiqeModel.fit`).  The file holds mu_pris_param [1,36] and
cov_pris_param [36,36], the keys of the Python ports' model file.  A model fitted here is not the release's modelparameters.mat
(which was fitted on halved images with overlapping blocks): scores against the two are not comparable.
Usage: python tools/niqe_fit.py --y4m CLIP.y4m [--step K] [--y4m_size WxH] [--y4m_matrix bt709] --out MODEL.npz"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--y4m", type=str, required=True, help="the clip, a YUV4MPEG2 file (8 to 16 bits)")
    ap.add_argument("--step", type=int, default=1, help="take every K-th frame")
    ap.add_argument("--y4m_size", type=str, default=None, help="WxH: resize on the device first, as evals.py --y4m_size does")
    ap.add_argument("--y4m_matrix", type=str, default="bt709", choices=["bt709", "bt601"])
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", type=str, required=True, help="MODEL.npz")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    videorun = importlib.import_module("zero-tig_amd.videorun")
    if a.step < 1:
        ap.error("--step is an integer >= 1; got %d" % a.step)
    if not os.path.isfile(a.y4m):
        ap.error("--y4m %s: no such file" % a.y4m)
    size = None
    if a.y4m_size is not None:
        size = videorun.parse_size(a.y4m_size)
        if size is None:
            ap.error("--y4m_size takes WxH, e.g. 1920x1080; got %r" % a.y4m_size)
    y4m = importlib.import_module("zero-tig_amd.y4m")
    grading = importlib.import_module("zero-tig_amd.grading")
    ops = importlib.import_module("zero-tig_amd.ops").Ops(importlib.import_module("zero-tig_amd.lib").get_lib())
    dev = torch.device("cuda", a.gpu)
    reader = y4m.Y4MReader(a.y4m)
    try:
        fmt = reader.header.format(a.y4m_matrix)
        if size is not None and tuple(size) == (fmt.W, fmt.H):
            size = None
        W, H = size or (fmt.W, fmt.H)
        if H < 96 or W < 96:
            raise SystemExit("the frames are %dx%d: NIQE needs at least one whole 96 x 96 block" % (W, H))
        payload = torch.empty(fmt.frame_bytes, dtype=torch.uint8, device=dev)
        rgb = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        bufs = ops.sized_bufs(fmt, size, dev) if size else None
        frames, n = [], 0
        for k, p in enumerate(reader):
            if k % a.step:
                continue
            payload.copy_(p, non_blocking=True)
            loaded = torch.cuda.Event()
            loaded.record()
            reader.release(loaded)
            if size is None:
                ops.yuv_to_planar_f32(payload, fmt, out=rgb)
            else:
                ops.yuv_to_planar_f32_sized(payload, fmt, size, out=rgb, bufs=bufs)
            si, sf = ops.niqe_block_sums(rgb)
            frames.append((si.cpu().numpy(), sf.cpu().numpy()))
            n += 1
    finally:
        reader.close()
    model = grading.NiqeModel.fit(frames, os.path.basename(a.out))
    model.save(a.out)
    print("%s: %d frames of %dx%d, %d sharp blocks of %d per frame taken, %d of them with all 36 features finite"
          % (a.out, n, W, H, model.blocks[1], (H // 96) * (W // 96), model.blocks[0]))


if __name__ == "__main__":
    main()
