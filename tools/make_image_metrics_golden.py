#!/usr/bin/env python3
"""Writes tests/golden/image_metrics.npz: for every case of tests/image_metrics_restatement.py (CASES) the fp32 inputs and what the REFERENCE's own
functions return for them — conerf/loss/ssim_torch.py's ssim(img1, img2), imported by path from a checkout of the reference, and its compute_psnr
(eval_ngp_nerf.py:24-27: F.mse_loss, then -10 log(mse + eps) / log 10, restated below because that file imports packages this project does not need).
Values are stored per image ([1,C,H,W] calls, as the reference's evaluator makes them).

    python tools/make_image_metrics_golden.py --reference <checkout of the reference>

CPU only; run once, where the reference is at hand.  No code of the reference is copied: only the numbers its functions return."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_metrics_restatement as IR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference checkout (contains conerf/loss/ssim_torch.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "image_metrics.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("_ref_ssim_torch", os.path.join(args.reference, "conerf", "loss", "ssim_torch.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    with torch.no_grad():
        for case in IR.CASES:
            name = case[0]
            pred, gt = IR.make_images(case)
            ssims, psnrs = [], []
            for i in range(pred.shape[0]):
                rgb = pred[i:i + 1].permute(0, 3, 1, 2)
                pixels = gt[i:i + 1].permute(0, 3, 1, 2)
                ssims.append(ref.ssim(pixels, rgb).item())                          # compute_ssim(pixels, rgb)
                mse = F.mse_loss(rgb, pixels)                                       # compute_psnr(rgb, pixels)
                psnrs.append((-10.0 * torch.log(mse + 1e-6) / np.log(10.0)).item())
            out[name + "/pred"], out[name + "/gt"] = pred.numpy(), gt.numpy()
            out[name + "/ssim"] = np.asarray(ssims, dtype=np.float32)
            out[name + "/psnr"] = np.asarray(psnrs, dtype=np.float32)
            print(f"{name}: ssim {ssims} psnr {psnrs}")
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
