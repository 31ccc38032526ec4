#!/usr/bin/env python3
"""Zero-TIG inference on MI355X -- same flags and outputs as the reference predict.py:23-36, 76-104."""
import argparse
import logging
import os
import json
import sys
import time

import numpy as np
import torch
import torch.utils.data
from PIL import Image

from dataloader.create_data import CreateDataset
from model.model import Finetunemodel
from utils import utils
from utils.utils import sequential_judgment

videorun = __import__("importlib").import_module("zero-tig_amd.videorun")

parser = argparse.ArgumentParser("ZERO-TIG")
parser.add_argument("--lowlight_images_path", type=str, default="./data")
parser.add_argument("--save", type=str, default="./results/")
parser.add_argument("--model_pretrain", type=str, default=r"./weights/BVI-RLV.pt")
parser.add_argument("--gpu", type=int, default=0)
parser.add_argument("--seed", type=int, default=2)
parser.add_argument("--of_scale", type=int, default=3)
parser.add_argument("--dataset", type=str, default="RLV")
parser.add_argument("--num_workers", type=int, default=-1, help="decode workers; -1: host cores - 2, at most 12")
parser.add_argument("--precision", type=str, default=None, choices=["fp32", "bf16"],
                    help="model precision: fp32 = parity mode, bf16 = throughput mode; when not given, ZEROTIG_PRECISION if set, else fp32")
parser.add_argument("--alternate_corr", type=int, default=0, choices=[0, 1],
                    help="RAFT's correlation (raft.py:39-40): 0 the all-pairs volume, 1 the on-the-fly lookup from the feature maps, "
                         "which forms no volume (DESIGN 8l: the volume grows with the fourth power of the frame side)")
parser.add_argument("--graph", type=int, default=0, choices=[0, 1],
                    help="1: drive the loop through InferStep (weights prepared once, steady-state frames replayed as one hipGraph)")


parser.add_argument("--device_png", type=int, default=0, choices=[0, 1, 2],
                    help="1: the result PNGs are deflated on the device and written by a threaded writer (same pixels, other file bytes); "
                         "2: the same with run-length matches, for frames with flat areas (never larger than 1)")
parser.add_argument("--timing_json", type=str, default=None,
                    help="write the loop's host-side time split (decode wait, step, copy wait, writer wait) to this file")
parser.add_argument("--y4m_in", type=str, default=None,
                    help="raw video in: a YUV4MPEG2 file, or - for standard input (8-bit C420jpeg / C420mpeg2 / C420paldv / C420 / C422 / "
                         "C444, or 9, 10, 12, 14 or 16 bits per sample as C420pN / C422pN / C444pN; progressive); replaces the dataset walk, one stream is one sequence; needs --graph 1.  The results "
                         "are written as <save>/<stem>_enhance.y4m and <stem>_denoise.y4m in the input's own layout")
parser.add_argument("--y4m_out", type=str, default=None,
                    help="write the enhance stream here instead (and no denoise stream); - is standard output, every log line then goes to stderr")
parser.add_argument("--y4m_resize", type=int, default=0, choices=[0, 1],
                    help="0: enhance at the stream's own size; 1: the loaders' resize((1920, 1080)) first, the output streams are 1920x1080")
parser.add_argument("--y4m_size", type=str, default=None,
                    help="WxH: enhance the stream at this size; the decoded frame is resized on the device in float (DESIGN 8g), at "
                         "every bit depth, and the output streams are W x H.  For weights trained with train.py --y4m_size; cannot be "
                         "combined with --y4m_resize 1; needs --y4m_in")
parser.add_argument("--y4m_out_depth", type=int, default=0, choices=[0, 8, 9, 10, 12, 14, 16],
                    help="bits per sample of the output streams; 0: as the input.  An 8-bit stream can leave as 10-bit (the model's fp32 "
                         "result keeps its gradation) and a deep one as 8-bit; needs --y4m_in")
parser.add_argument("--y4m_matrix", type=str, default="bt709", choices=["bt709", "bt601"],
                    help="the Y'CbCr matrix of the stream (Y4M cannot carry it)")
parser.add_argument("--y4m_scene_cut", type=float, default=0.0,
                    help="0: one stream is one sequence; T > 0: a frame whose scene score (DESIGN 8e: relative change of the luma's "
                         "16 x 16 cell sums against the previous frame, computed on the device on a stream of its own) exceeds T "
                         "starts a new sequence, i.e. the recurrent cache restarts there.  Suggested: 0.03, set from synthetic "
                         "clips only (cuts between unrelated low-light scenes), not validated on real footage")
parser.add_argument("--y4m_cuts_json", type=str, default=None,
                    help="write {threshold, cuts: [frame indices], score: [...], rel: [...]} here at the end; needs --y4m_scene_cut and --y4m_in")

def save_images(tensor):
    """predict.py:57-61: clip(x * 255, 0, 255).astype(uint8), HWC -- quantised and interleaved on the device (6 MB instead of
    25 MB per 1080p frame over PCIe)."""
    return utils.quantize_u8(tensor).cpu().numpy()


def main_y4m(args):
    """--y4m_in: frames come from a Y4M stream and leave as Y4M streams; the colour conversion runs inside the step (InferStep(yuv=))"""
    import importlib
    y4m = importlib.import_module("zero-tig_amd.y4m")
    sink = None
    if args.y4m_out == "-":                        # standard output carries the stream and nothing else: file descriptor 1 is
        sink = os.fdopen(os.dup(1), "wb")          # re-pointed at stderr for every print / log line, also of native code
        sys.stdout.flush()
        os.dup2(2, 1)
        sys.stdout = sys.stderr
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format="%(asctime)s %(message)s")
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", args.gpu)
    reader = y4m.Y4MReader(args.y4m_in)
    head = reader.header
    fmt = head.format(args.y4m_matrix)
    if fmt.depth > 8 and args.y4m_resize:
        reader.close()
        parser.error("--y4m_resize 1 cannot be combined with a %d-bit --y4m_in stream (C%s): the resize is 8-bit; --y4m_size WxH resizes "
                     "in float at any depth" % (fmt.depth, head.ctag))
    print("Y4M input: %dx%d C%s %d-bit %s %s" % (head.W, head.H, head.ctag, fmt.depth, "full" if head.full else "limited", args.y4m_matrix))
    out_depth = args.y4m_out_depth or fmt.depth
    if out_depth > 8 and fmt.depth == 8 and fmt.ss != 444 and fmt.siting == 0:
        logging.info("C%s -> C%s: the conversion keeps the centre siting of the input, which the output tag cannot express",
                     head.ctag, y4m.ctag_at_depth(head.ctag, out_depth))
    model = Finetunemodel(args).to(dev)
    model.eval()
    for p in model.parameters():
        p.requires_grad = False
    step = importlib.import_module("zero-tig_amd.infer").InferStep(model, use_graph=True, ingest_size=(1920, 1080) if args.y4m_resize else None,
                                                                   yuv=fmt, yuv_out_depth=out_depth, yuv_size=args.y4m_size)
    out_head = head.resized(step.yuv_format.W, step.yuv_format.H)._replace(ctag=y4m.ctag_at_depth(head.ctag, out_depth))
    det = None
    if args.y4m_scene_cut > 0:
        det = importlib.import_module("zero-tig_amd.scenecut").SceneCut(utils._ops(), dev, fmt, args.y4m_scene_cut)
    seq = videorun.Sequences(det, args.y4m_scene_cut)
    if args.y4m_out is not None:
        writers = [y4m.Y4MWriter(args.y4m_out, out_head, fh=sink)]
    else:
        os.makedirs(args.save, exist_ok=True)
        stem = "stdin" if args.y4m_in == "-" else os.path.splitext(os.path.basename(args.y4m_in))[0]
        writers = [y4m.Y4MWriter(os.path.join(args.save, stem + kind), out_head) for kind in ("_enhance.y4m", "_denoise.y4m")]
    clock = time.perf_counter
    t = {"decode_wait": 0.0, "step": 0.0, "copy_wait": 0.0, "write": 0.0}
    frames, t_first = 0, None
    try:
        with torch.no_grad():
            while True:
                t0 = clock()
                try:
                    payload = next(reader)
                except StopIteration:
                    break
                t1 = clock()
                t_first = t1 if t_first is None else t_first
                step(payload, seq.next(payload))
                reader.release(step.loaded)        # the ring buffer is free once the copy to the device has run
                t2 = clock()
                for w, p in zip(writers, step.yuv):    # the copies are ordered on the stream: the next step may overwrite the buffers
                    w.submit(p)
                t4 = clock()
                frames += 1
                t["decode_wait"] += t1 - t0
                t["step"] += t2 - t1
                t["write"] += t4 - t2
    finally:
        videorun.close_streams(writers, [reader])
    print("Total frame number: ", frames)
    if args.y4m_cuts_json:
        with open(args.y4m_cuts_json, "w") as fh:
            json.dump(seq.cuts_json(), fh)
    if args.timing_json and frames:
        t_end = clock()                            # the last stream has been closed
        t["writer_wait"] = sum(w.wait_writer for w in writers)
        t["write"] -= t["writer_wait"]
        # the writer threads' own time, summed over the streams: waiting for the step's event (the device) and inside write()
        t["writer_thread_event"] = sum(w.thread_event for w in writers)
        t["writer_thread_io"] = sum(w.thread_io for w in writers)
        extra = {}
        if det is not None:                        # part of `step`: the seconds pop() was blocked
            t["scene_wait"] = det.wait
            extra["cuts"] = len(seq.cuts)
        per = {k + "_ms": 1e3 * v / frames for k, v in t.items()}
        with open(args.timing_json, "w") as fh:
            json.dump(dict(per, frames=frames, seconds=t_end - t_first, fps=frames / (t_end - t_first), device_png=0, graph=args.graph,
                           y4m=1, y4m_resize=args.y4m_resize, **extra), fh)


def main():
    args = parser.parse_args()
    if args.y4m_in is None and (args.y4m_out is not None or args.y4m_resize):
        parser.error("--y4m_out / --y4m_resize need --y4m_in")
    if args.y4m_size is not None:
        if args.y4m_in is None:
            parser.error("--y4m_size needs --y4m_in")
        if args.y4m_resize:
            parser.error("--y4m_size cannot be combined with --y4m_resize 1: the first is the float resize to WxH, the second the "
                         "loaders' 8-bit resize to 1920x1080")
        size = videorun.parse_size(args.y4m_size)
        if size is None:
            parser.error("--y4m_size takes WxH, e.g. 1920x1080; got %r" % args.y4m_size)
        args.y4m_size = size
    if args.y4m_out_depth and args.y4m_in is None:
        parser.error("--y4m_out_depth needs --y4m_in")
    if args.y4m_scene_cut < 0:
        parser.error("--y4m_scene_cut is a threshold in [0, 1], 0 = off; got %g" % args.y4m_scene_cut)
    if args.y4m_scene_cut > 0 and args.y4m_in is None:
        parser.error("--y4m_scene_cut needs --y4m_in")
    if args.y4m_cuts_json is not None and not (args.y4m_scene_cut > 0 and args.y4m_in is not None):
        parser.error("--y4m_cuts_json needs --y4m_scene_cut T (T > 0) and --y4m_in")
    if args.y4m_in is not None:
        if not args.graph:
            parser.error("--y4m_in needs --graph 1 (the colour conversion runs inside InferStep); --graph is %d" % args.graph)
        if args.device_png:
            parser.error("--y4m_in writes Y4M streams, not PNG files: --device_png %d cannot be combined with it" % args.device_png)
        return main_y4m(args)
    os.makedirs(args.save, exist_ok=True)
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format="%(asctime)s %(message)s")
    # Finetunemodel builds its RAFT after the weights file is read (model.py:268-290), i.e. with freshly drawn weights: seed them,
    # as evals.py does, so that two runs over one weights file write the same images
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", args.gpu)
    args.device_ingest = True                      # loaders decode only; resize + ToTensor (multi_read_data.py:127-132) on the GPU
    test_set = CreateDataset(args, task="test")
    queue = torch.utils.data.DataLoader(test_set, batch_size=1, **utils.loader_kwargs(utils.loader_workers(args.num_workers)))
    print("Total image number: ", len(test_set))
    model = Finetunemodel(args).to(dev)
    model.eval()
    for p in model.parameters():
        p.requires_grad = False
    step = None
    if args.graph:
        import importlib
        step = importlib.import_module("zero-tig_amd.infer").InferStep(model, use_graph=True, ingest_size=(1920, 1080), png=args.device_png)
    writer = utils.png_writer() if args.device_png else None
    clock = time.perf_counter
    t = {"decode_wait": 0.0, "step": 0.0, "copy_wait": 0.0, "write": 0.0}
    frames, t_first = 0, None
    try:
        with torch.no_grad():
            it = iter(queue)
            while True:
                t0 = clock()
                try:
                    inp, img_name, img_path, last_img_path = next(it)
                except StopIteration:
                    break
                t1 = clock()
                t_first = t1 if t_first is None else t_first      # the first frame has been read
                i, frames = frames, frames + 1
                new_seq = i == 0 or sequential_judgment(img_path[0], last_img_path[0])
                if step is not None:               # the two uint8 images are made inside the step; valid until the next call
                    step(inp, new_seq)
                    enh_dev, out_dev = step.u8
                    if writer is not None:
                        enh_png, out_png = step.png
                else:
                    model.is_new_seq = new_seq
                    enhance, output, illum = model(utils.ingest_frame(inp, dev))
                    enh_dev, out_dev = utils.quantize_u8(enhance), utils.quantize_u8(output)   # predict.py:57-61 save_images
                    if writer is not None:
                        enh_png, out_png = utils.png_encode(enh_dev, args.device_png), utils.png_encode(out_dev, args.device_png)
                t2 = clock()
                if writer is None:
                    enh_u8, out_u8 = enh_dev.cpu().numpy(), out_dev.cpu().numpy()
                t3 = clock()
                if "RLV" == args.dataset:
                    parts = img_path[0].split(os.sep)
                    save_dir = os.path.join(args.save, parts[-3], parts[-2])
                else:
                    save_dir = os.path.join(args.save, os.path.basename(os.path.split(img_path[0])[0]))
                os.makedirs(save_dir, exist_ok=True)
                name = img_name[0].split("/")[-1].split(".")[0]
                if writer is None:
                    Image.fromarray(out_u8).save(save_dir + "/" + name + "_denoise.png", "PNG")
                    Image.fromarray(enh_u8).save(save_dir + "/" + name + "_enhance.png", "PNG")
                else:                              # the copies are ordered on the stream: the next step may overwrite the buffers
                    H, W = int(out_dev.shape[0]), int(out_dev.shape[1])
                    writer.submit([(save_dir + "/" + name + "_denoise.png", out_png[0], out_png[1], H, W),
                                   (save_dir + "/" + name + "_enhance.png", enh_png[0], enh_png[1], H, W)])
                t4 = clock()
                t["decode_wait"] += t1 - t0
                t["step"] += t2 - t1
                t["copy_wait"] += t3 - t2
                t["write"] += t4 - t3
    finally:
        if writer is not None:
            writer.close()
    if args.timing_json and frames:
        t_end = clock()                            # the last file has been closed
        if writer is not None:                     # submit = wait for the byte counts (the step) + wait for a free buffer
            t["copy_wait"] += writer.wait_copy
            t["writer_wait"] = writer.wait_writer
            t["write"] -= writer.wait_copy + writer.wait_writer
        per = {k + "_ms": 1e3 * v / frames for k, v in t.items()}
        with open(args.timing_json, "w") as fh:
            json.dump(dict(per, frames=frames, seconds=t_end - t_first, fps=frames / (t_end - t_first), device_png=args.device_png,
                           graph=args.graph), fh)


if __name__ == "__main__":
    main()
