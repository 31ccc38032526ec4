#!/usr/bin/env python3
"""Inference + PSNR / SSIM against ground truth, before and after histogram matching -- the reference evals.py (flags
evals.py:26-39, loop 107-170, metrics 83-87, matching 100-103, summary 184-192) with every metric computed on the device: PSNR
as an exact integer reduction, SSIM from integer window sums in fp64, histogram matching (all channels pooled, as skimage's
default does it) by a radix sort of the output.  LPIPS (VGG, evals.py:73-80, 92-98) is computed when --lpips_weights names the
user's `lpips.LPIPS(net='vgg').state_dict()` file (zero-tig_amd/lpips.py); without it the two LPIPS fields are null.
Ground truth: `<...>/input/<scene>/low_light_*/N.png` -> `<...>/gt/<scene>/normal_light_*/N.png` (evals.py:122)."""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch
import torch.utils.data
from PIL import Image

from dataloader.create_data import CreateDataset
from model.model import Finetunemodel
from utils import utils

parser = argparse.ArgumentParser("ZERO-IG")
parser.add_argument("--lowlight_images_path", type=str, default="./lowlight_dataset")
parser.add_argument("--save", type=str, default="./results/BVI-RLV")
parser.add_argument("--model_pretrain", type=str, default=r"./weights_1.pt")
parser.add_argument("--gpu", type=int, default=0)
parser.add_argument("--seed", type=int, default=2)
parser.add_argument("--of_scale", type=int, default=3)
parser.add_argument("--dataset", type=str, default="RLV")
parser.add_argument("--gain", type=int, default=100, help="kept for CLI compatibility (unused upstream as well)")
parser.add_argument("--save_images", type=int, default=20, help="write the first N result pairs (evals.py:162)")
parser.add_argument("--hist_match", type=int, default=1, help="0: skip histogram matching and the *_HM metrics (evals.py:114)")
parser.add_argument("--lpips_weights", type=str, default=None,
                    help="torch.save(lpips.LPIPS(net='vgg').state_dict(), FILE); default: no LPIPS (fields null)")
parser.add_argument("--lpips_precision", type=str, default="fp32", choices=["fp32", "bf16"])
parser.add_argument("--precision", type=str, default=None, choices=["fp32", "bf16"],
                    help="model precision: fp32 = parity mode, bf16 = throughput mode; when not given, ZEROTIG_PRECISION if set, else fp32")
parser.add_argument("--graph", type=int, default=0, choices=[0, 1],
                    help="1: drive the loop through InferStep (weights prepared once, steady-state frames replayed as one hipGraph)")
parser.add_argument("--device_png", type=int, default=0, choices=[0, 1, 2],
                    help="1: the --save_images files are deflated on the device and written by a threaded writer (same pixels); "
                         "2: the same with run-length matches, for frames with flat areas (never larger than 1)")


def main():
    args = parser.parse_args()
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
        json.dump({"Total_PSNR": total / max(n, 1), "Total_SSIM": total_ssim / max(n, 1),
                   "Total_LPIPS": total_lpips / max(n, 1) if lp_on else None,
                   "Total_PSNR_HM": total_hm / max(n, 1) if hm_on else None, "Total_SSIM_HM": total_ssim_hm / max(n, 1) if hm_on else None,
                   "Total_LPIPS_HM": total_lpips_hm / max(n, 1) if lp_on and hm_on else None, "images": n}, fh)


if __name__ == "__main__":
    main()
