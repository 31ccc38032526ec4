#!/usr/bin/env python3
"""Inference + PSNR / SSIM against ground truth, before and after histogram matching -- the reference evals.py (flags
evals.py:26-39, loop 107-170, metrics 83-87, matching 100-103, summary 184-192) with every metric computed on the device: PSNR
as an exact integer reduction, SSIM from integer window sums in fp64, histogram matching (all channels pooled, as skimage's
default does it) by a radix sort of the output.  LPIPS (VGG, evals.py:73-80, 92-98) is computed when --lpips_weights names the
user's `lpips.LPIPS(net='vgg').state_dict()` file (zero-tig_amd/lpips.py); without it the two LPIPS fields are null.
Ground truth: `<...>/input/<scene>/low_light_*/N.png` -> `<...>/gt/<scene>/normal_light_*/N.png` (evals.py:122)."""
import argparse
import importlib
import json
import logging
import math
import os
import sys
import time
import types

import numpy as np
import torch
import torch.utils.data
from PIL import Image

from dataloader.create_data import CreateDataset
from model.model import Finetunemodel
from utils import utils

grading = importlib.import_module("zero-tig_amd.grading")
scenecut = importlib.import_module("zero-tig_amd.scenecut")
videorun = importlib.import_module("zero-tig_amd.videorun")
loe50_grid, noref_values, NR_KEYS = grading.loe50_grid, grading.noref_values, grading.NR_KEYS
color_values, COLOR_KEYS = grading.color_values, grading.COLOR_KEYS

parser =argparse.ArgumentParser("ZERO-IG")
parser.add_argument("--lowlight_images_path", type=str, default="./lowlight_dataset")
parser.add_argument("--save", type=str, default="./results/BVI-RLV")
parser.add_argument("--model_pretrain", type=str, default=r"./weights_1.pt")
parser.add_argument("--gpu", type=int, default=0)
parser.add_argument("--seed", type=int, default=2)
parser.add_argument("--of_scale", type=int, default=3)
parser.add_argument("--dataset", type=str, default="RLV")
parser.add_argument("--gain", type=int, default=100, help="kept for CLI compatibility (unused upstream as well)")
parser.add_argument("--save_images", type=int, default=None, help="write the first N result pairs (evals.py:162); default 20")
parser.add_argument("--hist_match", type=int, default=None,
                    help="0: skip histogram matching and the *_HM metrics (evals.py:114); default 1 (with --noref 1 there is nothing to match)")
parser.add_argument("--lpips_weights", type=str, default=None,
                    help="torch.save(lpips.LPIPS(net='vgg').state_dict(), FILE); default: no LPIPS (fields null)")
parser.add_argument("--lpips_precision", type=str, default="fp32", choices=["fp32", "bf16"])
parser.add_argument("--precision", type=str, default=None, choices=["fp32", "bf16"],
                    help="model precision: fp32 = parity mode, bf16 = throughput mode; when not given, ZEROTIG_PRECISION if set, else fp32")
parser.add_argument("--alternate_corr", type=int, default=0, choices=[0, 1],
                    help="RAFT's correlation (raft.py:39-40): 0 the all-pairs volume, 1 the on-the-fly lookup from the feature maps, "
                         "which forms no volume (DESIGN 8l: the volume grows with the fourth power of the frame side)")
parser.add_argument("--graph", type=int, default=0, choices=[0, 1],
                    help="1: drive the loop through InferStep (weights prepared once, steady-state frames replayed as one hipGraph)")
parser.add_argument("--device_png", type=int, default=0, choices=[0, 1, 2],
                    help="1: the --save_images files are deflated on the device and written by a threaded writer (same pixels); "
                         "2: the same with run-length matches, for frames with flat areas (never larger than 1)")
parser.add_argument("--y4m_in", type=str, default=None,
                    help="raw video in: the low-light YUV4MPEG2 file, or - for standard input (the layouts of predict.py --y4m_in, 8 to 16 "
                         "bits); with --y4m_gt it replaces the dataset walk: the stream is enhanced as by predict.py --y4m_in and every "
                         "frame is graded against the frame of --y4m_gt; needs --graph 1")
parser.add_argument("--y4m_gt", type=str, default=None,
                    help="the ground-truth YUV4MPEG2 file (a file, not -): as many frames as --y4m_in, the same size after --y4m_size; "
                         "with the layout of the denoise stream (size, subsampling, depth) the plane metrics are reported as well")
parser.add_argument("--y4m_out", type=str, default=None, help="also write the enhance stream to this file while evaluating")
parser.add_argument("--y4m_size", type=str, default=None,
                    help="WxH: both streams are decoded at their own size and resized on the device in float (DESIGN 8g) before the model "
                         "and the RGB metrics; needs --y4m_in")
parser.add_argument("--y4m_out_depth", type=int, default=0, choices=[0, 8, 9, 10, 12, 14, 16],
                    help="bits per sample of the enhance / denoise payloads; 0: as the input; needs --y4m_in")
parser.add_argument("--y4m_matrix", type=str, default="bt709", choices=["bt709", "bt601"],
                    help="the Y'CbCr matrix of both streams (Y4M cannot carry it)")
parser.add_argument("--y4m_scene_cut", type=float, default=0.0,
                    help="0: one stream is one sequence; T > 0: a frame of --y4m_in whose scene score (DESIGN 8e) exceeds T starts a new "
                         "sequence, as in predict.py")
parser.add_argument("--y4m_cuts_json", type=str, default=None,
                    help="write {threshold, cuts: [frame indices], score: [...], rel: [...]} here at the end; needs --y4m_scene_cut and --y4m_in")
parser.add_argument("--timing_json", type=str, default=None,
                    help="with --y4m_in: write the loop's host-side time split per frame (decode wait, step, metric launches, table "
                         "read-backs, writer) and its frames per second to this file")
parser.add_argument("--y4m_frames_json", type=str, default=None,
                    help="write one record per frame here (plane SSEs and SSIMs, the RGB metrics, the cut flag); needs --y4m_in")
parser.add_argument("--tc", type=int, default=0, choices=[0, 1],
                    help="1: temporal consistency (DESIGN 8i): per frame pair of a sequence the warping error (Lai et al. 2018, occlusion "
                         "test of Ruder et al. 2016), the plain frame difference and MABD (Jiang and Zheng 2019) of the denoise result, "
                         "next to the same numbers of the ground truth; flows from RAFT on the ground-truth frames; needs --y4m_in")
parser.add_argument("--noref", type=int, default=0, choices=[0, 1],
                    help="1: grade --y4m_in without ground truth (DESIGN 8j): per frame the lightness order error of the denoise result "
                         "against the decoded input (LOE at full resolution, LOE_50 on the 50-pixel grid of the papers' tables), the mean "
                         "lightness of both and its gain, the entropies of the two lightness histograms and the saturated / black shares "
                         "of the result, under \"noref\" in Metrics.json; takes no --y4m_gt; with --tc 1 the flows come from RAFT on the "
                         "denoise result itself; needs --y4m_in")
parser.add_argument("--color", type=int, default=0, choices=[0, 1],
                    help="1: no-reference colour measures (DESIGN 8m), under \"color\" in Metrics.json: UIQM with its parts UICM / UISM / "
                         "UIConM (Panetta et al. 2016), UCIQE with its parts (Yang and Sowmya 2015), Hasler-Suesstrunk colourfulness and "
                         "the mean RGB level; with --y4m_in of the denoise result (\"out\"), of the decoded input (\"in\") and, with "
                         "--y4m_gt, of the ground truth (\"gt\"); in dataset mode of the result and the ground truth of each pair")
parser.add_argument("--color_block", type=int, default=None,
                    help="the side B of the blocks of UISM and UIConM, 4..64; default 10; the rows and columns beyond the last whole "
                         "block are in no block; needs --color 1")
parser.add_argument("--niqe", type=str, default=None,
                    help="MODEL.npz: NIQE (Mittal et al. 2013; DESIGN 8n), under \"niqe\" in Metrics.json, against the pristine model in "
                         "the file (mu_pris_param [36], cov_pris_param [36,36], as the Python ports keep it and as tools/niqe_fit.py "
                         "writes it from footage of your own; the MATLAB release's .mat with scipy): with --y4m_in of the denoise result "
                         "(\"out\"), of the decoded input (\"in\") and, with --y4m_gt, of the ground truth (\"gt\"); in dataset mode of "
                         "the result and the ground truth of each pair; frames with fewer than two whole 96 x 96 blocks give null")
parser.add_argument("--tc_scale", type=int, default=None,
                    help="integer S >= 1: the temporal metrics are taken at (H // S, W // S); default --of_scale; needs --tc 1")
parser.add_argument("--tc_raft_weights", type=str, default=None,
                    help="a RAFT state dict in the reference's key names (a module. prefix is accepted) for the flows of --tc 1, e.g. "
                         "trained RAFT weights of your own.  Default: the raft.* tensors of the model as --model_pretrain leaves them; as "
                         "in the reference, RAFT is never trained there and is built after the weights file is read, so unless your "
                         "checkpoint was made to hold a trained RAFT these are freshly drawn weights (seeded by --seed) and the warping "
                         "error measures little; needs --tc 1")
parser.add_argument("--tc_alternate_corr", type=int, default=None, choices=[0, 1],
                    help="the correlation path of the two RAFT runs of --tc 1 (see --alternate_corr); default: the value of "
                         "--alternate_corr; needs --tc 1")
parser.add_argument("--tc_viz", type=str, default=None,
                    help="PATH.y4m: one diagnostic picture per frame (DESIGN 8k), 2w x 2h at the reduced size of --tc_scale, 8-bit C420 "
                         "limited range: the colour wheel of the backward and of the forward flow, the denoise result with the pixels "
                         "that leave the frame in magenta and those that fail the forward-backward test in cyan, and the warping "
                         "error of the valid pixels in grey; the first frame of a sequence has white flow panels; needs --tc 1")
parser.add_argument("--tc_viz_max", type=float, default=None,
                    help="0 (default): each pair's flows are drawn at the scale of their joint largest radius; R > 0: R pixels of the "
                         "reduced frame are full saturation in every picture, longer flows are drawn at 0.75 brightness; needs --tc_viz")
parser.add_argument("--tc_viz_gain", type=float, default=None,
                    help="the grey of the error panel is min(1, sqrt(e / 3) * G); default 4; needs --tc_viz")
parser.add_argument("--tc_flo_dir", type=str, default=None,
                    help="per graded pair write DIR/%%06d_bwd.flo (current -> previous) and DIR/%%06d_fwd.flo (previous -> current), "
                         "Middlebury .flo files at the reduced size, in reduced-frame pixels, numbered by the current frame; needs --tc 1")

CHUNK = 64                                         # frames per read-back of the metric table


def check_y4m_args(args):
    """every argument check of the video mode, before anything touches the device -> True when the video mode was asked for"""
    if args.color_block is not None and not args.color:
        parser.error("--color_block needs --color 1")
    if args.color:
        args.color_block = 10 if args.color_block is None else args.color_block
        if not 4 <= args.color_block <= 64:
            parser.error("--color_block is the side of a block in pixels, 4..64; got %d" % args.color_block)
    if args.niqe is not None and not os.path.isfile(args.niqe):
        parser.error("--niqe %s: no such file (a pristine model, .npz with mu_pris_param and cov_pris_param; tools/niqe_fit.py "
                     "fits one)" % args.niqe)
    explicit_hm = args.hist_match is not None
    if not explicit_hm:
        args.hist_match = 0 if args.noref else 1
    if args.noref:
        if args.y4m_in is None:
            parser.error("--noref 1 needs --y4m_in: it grades a raw video against its own input")
        if args.y4m_gt is not None:
            parser.error("--noref 1 grades without ground truth: --y4m_gt cannot be combined with it")
        if args.lpips_weights is not None:
            parser.error("--noref 1 grades without ground truth: --lpips_weights cannot be combined with it (LPIPS needs --y4m_gt)")
        if explicit_hm and args.hist_match:
            parser.error("--noref 1 grades without ground truth: --hist_match %d cannot be combined with it (there is no histogram "
                         "to match)" % args.hist_match)
    if not args.tc:
        for flag in ("tc_scale", "tc_raft_weights", "tc_alternate_corr", "tc_viz", "tc_viz_max", "tc_viz_gain", "tc_flo_dir"):
            if getattr(args, flag) is not None:
                parser.error("--%s needs --tc 1" % flag)
    if args.tc_viz is None:
        for flag in ("tc_viz_max", "tc_viz_gain"):
            if getattr(args, flag) is not None:
                parser.error("--%s needs --tc_viz" % flag)
    if args.y4m_in is None:
        if args.tc:
            parser.error("--tc 1 needs --y4m_in")
        for flag in ("y4m_gt", "y4m_out", "y4m_size", "y4m_cuts_json", "y4m_frames_json", "timing_json"):
            if getattr(args, flag) is not None:
                parser.error("--%s needs --y4m_in" % flag)
        if args.y4m_out_depth:
            parser.error("--y4m_out_depth needs --y4m_in")
        if args.y4m_scene_cut != 0:
            parser.error("--y4m_scene_cut needs --y4m_in")
        return False
    if args.y4m_gt is None and not args.noref:
        parser.error("--y4m_in needs --y4m_gt: the ground-truth stream the frames are graded against")
    if args.y4m_gt == "-":
        parser.error("--y4m_gt must be a file: only --y4m_in can be read from standard input")
    if not args.graph:
        parser.error("--y4m_in needs --graph 1 (the colour conversion runs inside InferStep); --graph is %d" % args.graph)
    if args.device_png:
        parser.error("--y4m_in writes Y4M streams, not PNG files: --device_png %d cannot be combined with it" % args.device_png)
    if args.save_images is not None:
        parser.error("--y4m_in writes no image files: --save_images cannot be combined with it (--y4m_out FILE keeps the enhance stream)")
    if args.y4m_out == "-":
        parser.error("--y4m_out must be a file: standard output carries the log")
    if args.y4m_size is not None:
        size = videorun.parse_size(args.y4m_size)
        if size is None:
            parser.error("--y4m_size takes WxH, e.g. 1920x1080; got %r" % args.y4m_size)
        args.y4m_size = size
    if args.y4m_scene_cut < 0:
        parser.error("--y4m_scene_cut is a threshold in [0, 1], 0 = off; got %g" % args.y4m_scene_cut)
    if args.y4m_cuts_json is not None and not args.y4m_scene_cut > 0:
        parser.error("--y4m_cuts_json needs --y4m_scene_cut T (T > 0) and --y4m_in")
    if not args.noref and not os.path.isfile(args.y4m_gt):
        parser.error("--y4m_gt %s: no such file" % args.y4m_gt)
    if args.tc:
        if args.tc_scale is None:
            args.tc_scale = args.of_scale
        if args.tc_scale < 1:
            parser.error("--tc_scale is an integer >= 1; got %d" % args.tc_scale)
        if args.tc_alternate_corr is None:
            args.tc_alternate_corr = args.alternate_corr
        if args.tc_raft_weights is not None and not os.path.isfile(args.tc_raft_weights):
            parser.error("--tc_raft_weights %s: no such file" % args.tc_raft_weights)
        if args.tc_viz is not None:
            args.tc_viz_max = 0.0 if args.tc_viz_max is None else args.tc_viz_max
            args.tc_viz_gain = 4.0 if args.tc_viz_gain is None else args.tc_viz_gain
            if not (0 <= args.tc_viz_max < math.inf):
                parser.error("--tc_viz_max is a flow length in pixels >= 0, 0 = each pair at its own scale; got %g" % args.tc_viz_max)
            if not (0 <= args.tc_viz_gain < math.inf):
                parser.error("--tc_viz_gain is a factor >= 0; got %g" % args.tc_viz_gain)
            if args.tc_viz == "-":
                parser.error("--tc_viz must be a file: standard output carries the log")
            for flag in ("y4m_in", "y4m_gt", "y4m_out"):
                other = getattr(args, flag)
                if other not in (None, "-") and os.path.abspath(other) == os.path.abspath(args.tc_viz):
                    parser.error("--tc_viz %s is the file of --%s" % (args.tc_viz, flag))
    return True


class GroundTruth:
    """The ground-truth stream on the device: `load(payload)` copies a frame's payload into a static buffer (`loaded` is the event
    behind that copy) and decodes it the way InferStep decodes its input -- `Ops.yuv_to_planar_f32`, or
    `Ops.yuv_to_planar_f32_sized` when the streams are resized -- into `rgb` [1,3,H,W]; `payload` is the device copy."""

    def __init__(self, ops, fmt, size, dev):
        self.ops, self.fmt = ops, fmt
        self.size = None if size is None or tuple(size) == (fmt.W, fmt.H) else (int(size[0]), int(size[1]))
        W, H = self.size or (fmt.W, fmt.H)
        self.payload = torch.empty(fmt.frame_bytes, dtype=torch.uint8, device=dev)
        self.rgb = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        self._bufs = ops.sized_bufs(fmt, self.size, dev) if self.size else None
        self.loaded = None

    def load(self, payload):
        self.payload.copy_(payload, non_blocking=True)
        self.loaded = torch.cuda.Event()
        self.loaded.record()
        if self.size is None:
            return self.ops.yuv_to_planar_f32(self.payload, self.fmt, out=self.rgb)
        return self.ops.yuv_to_planar_f32_sized(self.payload, self.fmt, self.size, out=self.rgb, bufs=self._bufs)


def _plane_format(out_fmt, gt_fmt):
    """the layout the plane metrics are taken in, or None (one log line says why) when the two payloads cannot be compared"""
    why = None
    if (gt_fmt.W, gt_fmt.H, gt_fmt.ss, gt_fmt.depth) != (out_fmt.W, out_fmt.H, out_fmt.ss, out_fmt.depth):
        why = "the denoise payload is %dx%d %d %d-bit, the ground truth %dx%d %d %d-bit" % (
            out_fmt.W, out_fmt.H, out_fmt.ss, out_fmt.depth, gt_fmt.W, gt_fmt.H, gt_fmt.ss, gt_fmt.depth)
    elif min(out_fmt.chroma_shape) < 7 or min(out_fmt.H, out_fmt.W) < 7:
        why = "a plane is smaller than the 7 x 7 window of SSIM"
    if why is not None:
        logging.info("plane metrics off (planes: null): %s", why)
    return out_fmt if why is None else None


def _temporal(args, model, ops, dev, H, W):
    """--tc 1: the `TemporalConsistency` of the run, or None (the log says why) when the reduced frame is too small for RAFT"""
    temporal = importlib.import_module("zero-tig_amd.temporal")
    why = temporal.too_small(H, W, args.tc_scale)
    if why is not None:
        logging.info("temporal metrics off (temporal: null): %s", why)
        if args.tc_viz is not None or args.tc_flo_dir is not None:
            logging.info("temporal pictures off as well: %s are not written", " and ".join(
                n for n, v in (("--tc_viz " + str(args.tc_viz), args.tc_viz), ("the .flo files of --tc_flo_dir", args.tc_flo_dir))
                if v is not None))
        return None
    if args.tc_raft_weights is not None:
        raft_w = temporal.load_raft_weights(args.tc_raft_weights, model.raft.state_dict(), dev)
    else:
        raft_w = {"raft." + k: v.data for k, v in model.raft.state_dict().items()}
    return temporal.TemporalConsistency(ops, raft_w, dev, H, W, args.tc_scale, model.precision, keep_pair=args.tc_viz is not None,
                                        alternate_corr=bool(args.tc_alternate_corr))


def _read_rows(rows, graders, cut_flags, records):
    """the rows the table has read back, through every grader: the totals, the log lines and one record per frame"""
    for i, ri, rf in rows:
        rec = {"frame": i, "cut": cut_flags[i]}
        for g in graders:
            g.read(i + 1, rec, ri, rf)
        records.append(rec)


def main_y4m(args):
    """--y4m_in LOW --y4m_gt GT: the low stream through InferStep(yuv=) as in predict.py, every frame graded against the ground
    truth's; --y4m_in LOW --noref 1: the same loop without a ground-truth reader, every frame graded against its own decoded
    input.  Each grader's kernels write into a row of the metric table on the device; the table is read back every
    CHUNK frames (and at the end), one chunk late, so the host keeps running ahead of the device (zero-tig_amd/grading.py)."""
    y4m = importlib.import_module("zero-tig_amd.y4m")
    os.makedirs(args.save, exist_ok=True)
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format="%(asctime)s %(message)s", datefmt="%m/%d %I:%M:%S %p")
    logging.getLogger().addHandler(logging.FileHandler(os.path.join(args.save, "log.txt")))
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", args.gpu)
    noref = bool(args.noref)
    reader = y4m.Y4MReader(args.y4m_in)
    try:
        gt_reader = None if noref else y4m.Y4MReader(args.y4m_gt)
    except BaseException:
        reader.close()
        raise
    writer, viz_writer, flo_writer = None, None, None
    try:
        head = reader.header
        gt_head = head if noref else gt_reader.header
        fmt, gt_fmt = head.format(args.y4m_matrix), gt_head.format(args.y4m_matrix)
        for name, h, f in (("input", head, fmt),) + (() if noref else (("ground truth", gt_head, gt_fmt),)):
            logging.info("Y4M %s: %dx%d C%s %d-bit %s %s", name, h.W, h.H, h.ctag, f.depth, "full" if h.full else "limited", args.y4m_matrix)
        out_depth = args.y4m_out_depth or fmt.depth
        W, H = args.y4m_size or (fmt.W, fmt.H)
        if args.y4m_size is None and (gt_fmt.W, gt_fmt.H) != (W, H):
            raise ValueError("the streams differ in frame size: --y4m_in is %dx%d, --y4m_gt is %dx%d (--y4m_size WxH resizes both)"
                             % (fmt.W, fmt.H, gt_fmt.W, gt_fmt.H))
        model = Finetunemodel(args).to(dev)
        model.eval()
        for p in model.parameters():
            p.requires_grad = False
        step = importlib.import_module("zero-tig_amd.infer").InferStep(model, use_graph=True, ingest_size=None, yuv=fmt,
                                                                       yuv_out_depth=out_depth, yuv_size=args.y4m_size)
        ops = utils._ops()
        out_fmt = step.yuv_format
        gt = None if noref else GroundTruth(ops, gt_fmt, (W, H), dev)
        plane_fmt = None if noref else _plane_format(out_fmt, gt_fmt)      # --noref 1: no ground-truth payload to hold the planes against
        tc = _temporal(args, model, ops, dev, H, W) if args.tc else None
        tc_extra, viz, flo = {}, None, None
        if tc is not None and args.tc_viz is not None:
            viz_head = head.resized(2 * tc.w, 2 * tc.h)._replace(ctag="420mpeg2", color_range="LIMITED")
            viz_writer = y4m.Y4MWriter(args.tc_viz, viz_head)
            viz = (viz_writer, viz_head.format(args.y4m_matrix), args.tc_viz_max, args.tc_viz_gain)
            tc_extra["viz"] = {"path": args.tc_viz, "size": [2 * tc.w, 2 * tc.h], "max": args.tc_viz_max, "gain": args.tc_viz_gain}
        if tc is not None and args.tc_flo_dir is not None:
            os.makedirs(args.tc_flo_dir, exist_ok=True)
            flo_writer = importlib.import_module("zero-tig_amd.flowio").FloWriter()
            flo, tc_extra["flo_dir"] = (flo_writer, args.tc_flo_dir), args.tc_flo_dir
        pictures = grading.TemporalPictures(ops, tc, dev, viz, flo) if viz or flo else None
        det = scenecut.SceneCut(ops, dev, fmt, args.y4m_scene_cut) if args.y4m_scene_cut > 0 else None
        seq = videorun.Sequences(det, args.y4m_scene_cut)
        if args.y4m_out is not None:
            out_head = head.resized(out_fmt.W, out_fmt.H)._replace(ctag=y4m.ctag_at_depth(head.ctag, out_depth))
            writer = y4m.Y4MWriter(args.y4m_out, out_head)
        lpips_model = utils.lpips_model(args.lpips_weights, dev, args.lpips_precision) if args.lpips_weights else None
        hm_on, lp_on = bool(args.hist_match), lpips_model is not None

        tab = grading.MetricTable(dev, CHUNK)
        if noref:
            graders = [grading.NorefGrader(tab, ops, loe50_grid(H, W))]
        else:
            graders = [grading.RgbGrader(tab, ops, 3 * H * W, utils.histogram_match if hm_on else None, lpips_model),
                       grading.PlaneGrader(tab, ops, plane_fmt)]
        if args.tc:
            tc_meta = {"scale": args.tc_scale, "raft": "file" if args.tc_raft_weights else "checkpoint"}
            temporal_grader = grading.TemporalGrader(tab, tc, noref, tc_meta, tc_extra)
            graders.append(temporal_grader)
        if args.color:
            graders.append(grading.ColorGrader(tab, ops, args.color_block, ("out", "in") + (() if noref else ("gt",))))
        if args.niqe:
            graders.append(grading.NiqeGrader(tab, ops, grading.NiqeModel.load(args.niqe), ("out", "in") + (() if noref else ("gt",))))
        tab.build()
        ctx = types.SimpleNamespace(step=step, output=None, gt=None, gt_yuv=None if noref else gt.payload, cut=False)
        records, frames, t_first = [], 0, None
        clock = time.perf_counter
        t = {"decode_wait": 0.0, "step": 0.0, "metrics": 0.0, "readback": 0.0, "write": 0.0, "viz": 0.0}
        with torch.no_grad():
            while True:
                t0 = clock()
                payload = next(reader, None)
                gt_payload = payload if noref else next(gt_reader, None)
                if payload is None or gt_payload is None:
                    if payload is not None or gt_payload is not None:
                        # the longer stream is read to its end, so that the message names both lengths
                        n_in = frames + (0 if payload is None else 1 + sum(1 for _ in reader))
                        n_gt = frames + (0 if gt_payload is None else 1 + sum(1 for _ in gt_reader))
                        raise ValueError("the streams differ in length: --y4m_in has %d frames, --y4m_gt has %d" % (n_in, n_gt))
                    break
                t1 = clock()
                t_first = t1 if t_first is None else t_first
                ctx.cut = seq.next(payload)
                enhance, ctx.output, illum = step(payload, ctx.cut)
                reader.release(step.loaded)
                t2 = clock()
                if noref:                          # --tc 1: the flows come from the enhanced stream itself
                    ctx.gt = ctx.output
                else:
                    ctx.gt = gt.load(gt_payload)
                    gt_reader.release(gt.loaded)
                ri, rf = tab.row(frames)
                for g in graders:
                    g.launch(ctx, ri, rf)
                t_m = clock()
                if pictures is not None:
                    pictures.submit(frames, temporal_grader.flags[-1])
                t3 = clock()
                if writer is not None:
                    writer.submit(step.yuv[0])
                t4 = clock()
                frames += 1
                _read_rows(tab.advance(frames), graders, seq.flags, records)
                t5 = clock()
                t["decode_wait"] += t1 - t0
                t["step"] += t2 - t1
                t["metrics"] += t_m - t2
                t["viz"] += t3 - t_m
                t["write"] += t4 - t3
                t["readback"] += t5 - t4
            t5 = clock()
            _read_rows(tab.finish(), graders, seq.flags, records)
            t_end = clock()                        # every metric of the last frame has been read back
            t["readback"] += t_end - t5
    finally:
        videorun.close_streams((writer, viz_writer, flo_writer), (reader, gt_reader))
    result = dict.fromkeys(("Total_PSNR", "Total_SSIM", "Total_LPIPS", "Total_PSNR_HM", "Total_SSIM_HM", "Total_LPIPS_HM"))
    result.update(images=frames, planes=None)
    if noref:                                      # every key in its place before the graders fill theirs in
        result["noref"] = None
    if det is not None:
        result["cuts"] = seq.cuts
    if args.tc:
        result["temporal"] = None
    if args.color:
        result["color"] = None
    if args.niqe:
        result["niqe"] = None
    for g in graders:
        g.summary(result)
    with open(os.path.join(args.save, "Metrics.json"), "w") as fh:
        json.dump(result, fh)
    if args.y4m_frames_json:
        with open(args.y4m_frames_json, "w") as fh:
            json.dump(records, fh)
    if args.y4m_cuts_json:
        with open(args.y4m_cuts_json, "w") as fh:
            json.dump(seq.cuts_json(), fh)
    if args.timing_json and frames:
        per = {k + "_ms": 1e3 * v / frames for k, v in t.items() if k != "viz"}
        if pictures is not None:                   # the time `submit` waited for a free slot is part of viz_ms
            per["viz"] = {"viz_ms": 1e3 * t["viz"] / frames,
                          "wait_writer_ms": 1e3 * sum(w.wait_writer for w in (viz_writer, flo_writer) if w is not None) / frames}
        with open(args.timing_json, "w") as fh:
            json.dump(dict(per, frames=frames, seconds=t_end - t_first, fps=frames / (t_end - t_first), graph=args.graph, y4m=1,
                           hist_match=int(hm_on), lpips=int(lp_on), planes=int(plane_fmt is not None), **({"noref": 1} if noref else {}),
                           **({"color": 1} if args.color else {}), **({"niqe": 1} if args.niqe else {}),
                           scene_wait_ms=1e3 * det.wait / frames if det is not None else None,
                           **({"tc": int(tc is not None), "tc_scale": args.tc_scale} if args.tc else {})), fh)
    logging.info("Total frame number: %d", frames)



def main():
    args = parser.parse_args()
    if check_y4m_args(args):
        return main_y4m(args)
    if args.save_images is None:
        args.save_images = 20
    os.makedirs(args.save, exist_ok=True)
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format="%(asctime)s %(message)s", datefmt="%m/%d %I:%M:%S %p")
    logging.getLogger().addHandler(logging.FileHandler(os.path.join(args.save, "log.txt")))
    # Finetunemodel builds its RAFT after the weights file is read (model.py:268-290), i.e. with freshly drawn weights: seed them,
    # as train.py does, so that two evaluations of one weights file report the same numbers
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda", args.gpu)
    args.device_ingest = True                      # loaders decode only; resize + ToTensor (multi_read_data.py:127-132) on the GPU
    test_set = CreateDataset(args, task="test")
    queue = torch.utils.data.DataLoader(test_set, batch_size=1, **utils.loader_kwargs(utils.loader_workers(-1)))
    logging.info("Total image number: %d; model path = %s", len(test_set), args.model_pretrain)
    model = Finetunemodel(args).to(dev)
    model.eval()
    total, n = 0.0, 0
    total_ssim, total_hm, total_ssim_hm = 0.0, 0.0, 0.0
    lpips_model = utils.lpips_model(args.lpips_weights, dev, args.lpips_precision) if args.lpips_weights else None
    total_lpips, total_lpips_hm = 0.0, 0.0
    color_means, color_blocks = {"out": grading.ColorMeans(), "gt": grading.ColorMeans()}, None
    niqe_model = grading.NiqeModel.load(args.niqe) if args.niqe else None
    niqe_tot, niqe_count, niqe_blocks = {"out": 0.0, "gt": 0.0}, {"out": 0, "gt": 0}, None
    step = None
    if args.graph:
        import importlib
        step = importlib.import_module("zero-tig_amd.infer").InferStep(model, use_graph=True, ingest_size=(1920, 1080))
    writer = utils.png_writer() if args.device_png else None
    with torch.no_grad():
        for i, (inp, img_name, img_path, last_img_path) in enumerate(queue):
            new_seq = i == 0 or utils.sequential_judgment(img_path[0], last_img_path[0])
            if step is not None:                   # the tensors live in the step's buffers: everything below reads them before the next call
                enhance, output, illum = step(inp, new_seq)
            else:
                model.is_new_seq = new_seq
                enhance, output, illum = model(utils.ingest_frame(inp, dev))   # Finetunemodel.forward updates the recurrent cache itself
            gt_path = img_path[0].replace("input", "gt").replace("low_light_", "normal_light_")
            gt = torch.from_numpy(np.asarray(Image.open(gt_path).convert("RGB"), dtype=np.uint8).copy())
            gt_t = utils.ingest_frame(gt, dev)                     # same resize to 1920 x 1080 + ToTensor as the inputs, on the device
            psnr = utils.psnr(output, gt_t)                        # evals.py:83-85, exact integer sum on the device
            total, n = total + psnr, n + 1
            ssim = utils.ssim(output, gt_t)                        # evals.py:87
            total_ssim += ssim
            if lpips_model is None:
                logging.info("NUM: %d, PSNR: %.3f, SSIM: %.3f", n, psnr, ssim)
                logging.info("Total PSNR: %.3f, Total SSIM: %.3f", total / n, total_ssim / n)
            else:                                                  # evals.py:92-98, 153-157; the ground truth's features serve both calls
                gt_feat = lpips_model.features(gt_t)
                lp = utils.lpips(output, gt_feat, lpips_model)
                total_lpips += lp
                logging.info("NUM: %d, PSNR: %.3f, SSIM: %.3f, LPIPS: %.3f", n, psnr, ssim, lp)
                logging.info("Total PSNR: %.3f, Total SSIM: %.3f, Total LPIPS: %.3f", total / n, total_ssim / n, total_lpips / n)
            if args.hist_match:
                hm = utils.histogram_match(output, gt_t)           # evals.py:100-103, 158-159
                psnr_hm, ssim_hm = utils.psnr(hm, gt_t), utils.ssim(hm, gt_t)
                total_hm, total_ssim_hm = total_hm + psnr_hm, total_ssim_hm + ssim_hm
                if lpips_model is None:
                    logging.info("NUM: %d, PSNR_HM: %.3f, SSIM_HM: %.3f", n, psnr_hm, ssim_hm)
                    logging.info("Total PSNR_HM: %.3f, Total SSIM_HM: %.3f", total_hm / n, total_ssim_hm / n)
                else:                                              # evals.py:158-165: the float matched frame, not its quantised form
                    lp_hm = utils.lpips(hm, gt_feat, lpips_model)
                    total_lpips_hm += lp_hm
                    logging.info("NUM: %d, PSNR_HM: %.3f, SSIM_HM: %.3f, LPIPS_HM: %.3f", n, psnr_hm, ssim_hm, lp_hm)
                    logging.info("Total PSNR_HM: %.3f, Total SSIM_HM: %.3f, Total LPIPS_HM: %.3f", total_hm / n, total_ssim_hm / n,
                                 total_lpips_hm / n)
            if args.color:                                         # read back per image, as PSNR is
                color_blocks = [output.shape[2] // args.color_block, output.shape[3] // args.color_block]
                for which, frame in (("out", output), ("gt", gt_t)):
                    v = utils.color_quality(frame, args.color_block)
                    color_means[which].add(v)
                    logging.info("NUM: %d, color %s: %s", n, which, grading.color_text(v))
            if niqe_model is not None:                             # read back per image, as PSNR is
                niqe_blocks = [output.shape[2] // 96, output.shape[3] // 96]
                for which, frame in (("out", output), ("gt", gt_t)):
                    v = utils.niqe(frame, niqe_model)
                    if v is not None:
                        niqe_tot[which], niqe_count[which] = niqe_tot[which] + v, niqe_count[which] + 1
                    logging.info("NUM: %d, NIQE %s: %s", n, which, "null" if v is None else "%.4f" % v)
            if i < args.save_images:
                parts = img_path[0].split(os.sep)
                save_dir = os.path.join(args.save, parts[-3] + "/" + parts[-2])
                os.makedirs(save_dir, exist_ok=True)
                name = img_name[0].split("/")[-1].split(".")[0]
                imgs = [("_denoise.png", utils.quantize_u8(output)), ("_enhance.png", utils.quantize_u8(enhance))]
                if args.hist_match:                                # evals.py:178-181: np.round(x * 255), written as RGB
                    imgs.append(("_denoise_hm.png", utils.quantize_u8(hm, round_half_even=True)))
                if writer is None:
                    for suffix, u8 in imgs:
                        Image.fromarray(u8.cpu().numpy()).save(save_dir + "/" + name + suffix, "PNG")
                else:
                    writer.submit([(save_dir + "/" + name + suffix,) + tuple(utils.png_encode(u8, args.device_png)) + (u8.shape[0], u8.shape[1])
                                   for suffix, u8 in imgs])
    if writer is not None:
        writer.close()
    with open(os.path.join(args.save, "Metrics.json"), "w") as fh:
        hm_on = bool(args.hist_match)
        lp_on = lpips_model is not None
        result = {"Total_PSNR": total / max(n, 1), "Total_SSIM": total_ssim / max(n, 1),
                  "Total_LPIPS": total_lpips / max(n, 1) if lp_on else None,
                  "Total_PSNR_HM": total_hm / max(n, 1) if hm_on else None, "Total_SSIM_HM": total_ssim_hm / max(n, 1) if hm_on else None,
                  "Total_LPIPS_HM": total_lpips_hm / max(n, 1) if lp_on and hm_on else None, "images": n}
        if args.color:
            result["color"] = {"block": args.color_block, "graded": "denoise", "blocks": color_blocks, "out": color_means["out"].means(),
                               "in": None, "gt": color_means["gt"].means()}
            logging.info("colour (%d images, blocks of %d): out %s; gt %s", n, args.color_block,
                         grading.color_text(result["color"]["out"]), grading.color_text(result["color"]["gt"]))
        if niqe_model is not None:
            means = {w: niqe_tot[w] / niqe_count[w] if niqe_count[w] else None for w in ("out", "gt")}
            result["niqe"] = {"model": niqe_model.name, "blocks": niqe_blocks, "graded": "denoise", "out": means["out"], "in": None,
                              "gt": means["gt"], "frames_with_value": niqe_count}
            logging.info("NIQE (%d images, model %s): %s", n, niqe_model.name, ", ".join(
                "%s: %s" % (w, "null" if result["niqe"][w] is None else "%.4f" % result["niqe"][w]) for w in ("out", "gt")))
        json.dump(result, fh)


if __name__ == "__main__":
    main()
