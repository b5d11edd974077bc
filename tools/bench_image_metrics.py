#!/usr/bin/env python3
"""PSNR / SSIM of 12 views of 800 x 800 x 3: the fused kernel (dreg_nerf_amd.image_metrics, one call for all views) against the torch-composed path
on the same GPU — the reference's formula (five grouped 11x11 F.conv2d per view plus elementwise passes, conerf/loss/ssim_torch.py) with the data
movement of its evaluate() loop (eval_ngp_nerf.py:196-229: float images to the host, two uint8 conversions there, float images back, .item() per
metric).  The composed path is the baseline, not code under test.

  device time     hipEvent pairs around each path's launches for all 12 views, after warm-up, the two paths alternated, median of --rounds
  evaluator time  host clock around each path including its copies and synchronisations (what one block's evaluation pays besides rendering)

Writes one JSON object (--out, default profiles/image_metrics_bench.json).  Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dreg_nerf_amd import image_metrics as IM  # noqa: E402

VIEWS, H, W, C = 12, 800, 800, 3


def composed_ssim(img1, img2, window):
    """conerf/loss/ssim_torch.py's formula on [1,C,H,W] images."""
    c = img1.shape[1]
    mu1, mu2 = F.conv2d(img1, window, padding=5, groups=c), F.conv2d(img2, window, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img1 * img1, window, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(img2 * img2, window, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(img1 * img2, window, padding=5, groups=c) - mu1_mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean()


def composed_device(pred, gt, window):
    """The metrics alone, no copies: per view, results left on the device."""
    out = []
    for i in range(pred.shape[0]):
        a, b = pred[i:i + 1].permute(0, 3, 1, 2), gt[i:i + 1].permute(0, 3, 1, 2)
        mse = F.mse_loss(a, b)
        out.append((-10.0 * torch.log(mse + 1e-6) / np.log(10.0), composed_ssim(b, a, window)))
    return out


def composed_evaluator(pred, gt, window):
    """The reference's loop body without rendering, file writes and LPIPS."""
    rows = []
    for i in range(pred.shape[0]):
        rgb, pixels = pred[i].cpu().numpy(), gt[i].cpu().numpy()
        _u8 = (rgb * 255).astype(np.uint8), (pixels * 255).astype(np.uint8)
        a = torch.from_numpy(rgb[None, ...]).cuda().permute(0, 3, 1, 2)
        b = torch.from_numpy(pixels[None, ...]).cuda().permute(0, 3, 1, 2)
        mse = F.mse_loss(a, b)
        rows.append(((-10.0 * torch.log(mse + 1e-6) / np.log(10.0)).item(), composed_ssim(b, a, window).item()))
    return rows


def fused_evaluator(pred, gt):
    m = IM.image_metrics(pred, gt, return_u8=True)
    _u8 = m["pred_u8"].cpu().numpy(), m["gt_u8"].cpu().numpy()
    return list(zip(m["psnr"].cpu().tolist(), m["ssim"].cpu().tolist()))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_metrics.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    # the renderer's regime: a white background, a textured object in the middle, a small error on the object
    gt = torch.ones(VIEWS, H, W, C)
    gt[:, 200:600, 200:600] = torch.rand(VIEWS, 400, 400, C, generator=g)
    pred = gt.clone()
    pred[:, 200:600, 200:600] += 0.02 * torch.randn(VIEWS, 400, 400, C, generator=g)
    pred, gt = pred.clamp(0, 1).to(dev), gt.to(dev)
    window = IM.gaussian_taps().unsqueeze(1)
    window = window.mm(window.t())[None, None].expand(C, 1, 11, 11).contiguous().to(dev)

    paths = {
        "fused_device": lambda: IM.image_metrics(pred, gt),
        "fused_device_with_u8": lambda: IM.image_metrics(pred, gt, return_u8=True),
        "composed_device": lambda: composed_device(pred, gt, window),
    }
    walls = {"fused_evaluator": lambda: fused_evaluator(pred, gt), "composed_evaluator": lambda: composed_evaluator(pred, gt, window)}
    for _ in range(args.warmup):
        for fn in list(paths.values()) + list(walls.values()):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in list(paths) + list(walls)}
    for _ in range(args.rounds):                                  # alternated: drift of the box hits every path alike
        for k, fn in paths.items():
            times[k].append(event_ms(fn))
        for k, fn in walls.items():
            times[k].append(wall_ms(fn))
    fused, comp = fused_evaluator(pred, gt), composed_evaluator(pred, gt, window)
    agree = {"psnr_max_abs_diff_db": max(abs(a[0] - b[0]) for a, b in zip(fused, comp)), "ssim_max_abs_diff": max(abs(a[1] - b[1]) for a, b in zip(fused, comp))}
    res = {"views": VIEWS, "height": H, "width": W, "channels": C, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ms_all_views": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
           "agreement_fused_vs_composed": agree, "psnr_view0": fused[0][0], "ssim_view0": fused[0][1]}
    med = {k: v["median"] for k, v in res["ms_all_views"].items()}
    res["ms_per_view"] = {k: v / VIEWS for k, v in med.items()}
    res["speedup_device"] = med["composed_device"] / med["fused_device"]
    res["speedup_evaluator"] = med["composed_evaluator"] / med["fused_evaluator"]
    # input traffic floor of the fused call: both images read once
    res["fused_device_input_GBps"] = 2 * VIEWS * H * W * C * 4 / (med["fused_device"] * 1e-3) / 1e9
    assert all(math.isfinite(v) for v in med.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
