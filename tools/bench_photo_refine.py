#!/usr/bin/env python3
"""Photometric pose refinement on one MI355X: a generated block (the pose-recoverable fixture of
tests/test_hip_field_input_grad.py: smooth dense coarse levels, zero fine levels) with a 128^3 ball-shaped occupancy grid, source = target,
ground truth the identity.  First measurements: no ratio was set in advance, no default was tuned.

  phases     ms per iteration of one direction (4,096 rays, symmetric=False), hipEvent pairs, median of --steps after --warmup: the target render
             (render_image), the list forward + sort (dreg_ngp_render_train_samples, canonical_order), dreg_ngp_samples_grad,
             dreg_ngp_points_input_grad, dreg_ngp_samples_ray_grad, each called by hand on one iteration's rays; `step` = one event pair around
             PhotoRefiner.step() (measured, not a sum); `torch` = step minus the five (the pose chain, the loss, autograd, Adam: derived)
  kernel     dreg_ngp_points_input_grad alone at 2^18 points beside dreg_ngp_points_bwd on the same points, same process
  accuracy   final RRE / RTE of refine_pose_photometric at its defaults from 0.5 / 1 / 2 / 3 / 5 degree starts with |t| = 1 % of the angle in degrees
             (tools/bench_icp.py's starts)

Writes one JSON object (--out, default profiles/photo_refine_bench.json).  Needs a GPU."""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_hip_field_input_grad as G  # noqa: E402
from dreg_nerf_amd import field_train, ngp, ngp_train, photo_refine as PR, render as R  # noqa: E402

STARTS_DEG = (0.5, 1.0, 2.0, 3.0, 5.0)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def block(dev, res):
    f, _ = G.fixture_block()
    f = copy.deepcopy(f).to(dev).eval()
    grid = ngp.OccupancyGrid(G.FIX_AABB, res).to(dev)
    c = (torch.stack(torch.meshgrid(*[torch.arange(res)] * 3, indexing="ij"), -1).float() + 0.5) / res * 3.0 - 1.5
    grid._binary = (c.norm(dim=-1) < 0.8).to(dev)
    return f, grid, G.fixture_meta()


def start_pose(deg):
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    tdir = np.array([0.5, -0.7, 0.4]) / np.linalg.norm([0.5, -0.7, 0.4])
    return PR.se3_exp(torch.tensor(np.concatenate([np.radians(deg) * axis, 0.01 * deg * tdir]), dtype=torch.float64))


def phases(blk, dev, n_rays, steps, warmup):
    f, grid, meta = blk
    ref = PR.PhotoRefiner(blk, blk, start_pose(2.0), G.FIX_CAMS, G.FIX_CAMS, G.FIX_K, G.FIX_W, G.FIX_H, n_rays=n_rays, symmetric=False)
    f.requires_grad_(False)
    parts = R._grid_parts(grid, dev)
    bk = torch.tensor(PR.BKGD)
    names = ("target_render", "list_forward_sort", "samples_grad", "points_input_grad", "samples_ray_grad", "step")
    ts = {k: [] for k in names}
    n_samples = []
    for it in range(warmup + steps):
        ms_step, _ = event_ms(ref.step)
        with torch.no_grad():
            rays = PR.sample_camera_rays(ref.cams[1], G.FIX_K, G.FIX_W, G.FIX_H, n_rays, torch.Generator(device=dev).manual_seed(it))
            moved = PR.rays_to_block_diff(rays, PR.se3_exp(ref.xi.detach()) @ ref.G0)
            o, d = moved.origins.contiguous(), moved.viewdirs.contiguous()
            jitter = torch.zeros(n_rays, device=dev)
            cap = ngp_train.default_sample_capacity(n_rays, G.FIX_AABB, G.FIX_DT)
            ms_t, _ = event_ms(lambda: R.render_image(f, grid, rays, G.FIX_AABB, render_step_size=G.FIX_DT, render_bkgd=bk))

            def fwd():
                rgb, op, dep, rec, count = ngp_train.render_train_samples(f, parts, o, d, jitter, G.FIX_AABB, G.FIX_DT, list(PR.BKGD), 0.0, cap)
                return rgb, op, dep, ngp_train.canonical_order(rec, count), count
            ms_f, (rgb, op, dep, srt, count) = event_ms(fwd)
            g_rgb, g_dep = torch.randn_like(rgb) / n_rays, torch.randn_like(dep) / n_rays
            ms_g, grads = event_ms(lambda: ngp_train.samples_grad(srt, d, rgb, op, dep, g_rgb, None, g_dep, G.FIX_DT))
            ms_i, (gx, gdir) = event_ms(lambda: field_train.points_input_grad(f, srt["x"], grads[0], grads[1], grads[2]))
            go, gd = torch.empty(n_rays, 3, device=dev), torch.empty(n_rays, 3, device=dev)
            from dreg_nerf_amd import lib as L
            ms_r, _ = event_ms(lambda: L.check(L.load().dreg_ngp_samples_ray_grad(count, L.ptr(srt["ray"]), L.ptr(srt["t"]), L.ptr(gx), L.ptr(gdir), n_rays,
                                                                                  L.ptr(go), L.ptr(gd), L.stream()), "dreg_ngp_samples_ray_grad"))
        if it >= warmup:
            for k, v in zip(names, (ms_t, ms_f, ms_g, ms_i, ms_r, ms_step)):
                ts[k].append(v)
            n_samples.append(count)
    f.requires_grad_(True)
    out = {k: round(statistics.median(v), 4) for k, v in ts.items()}
    out["torch_derived"] = round(out["step"] - sum(out[k] for k in names[:5]), 4)
    out["samples_per_iteration_median"] = int(statistics.median(n_samples))
    ref2 = PR.PhotoRefiner(blk, blk, start_pose(2.0), G.FIX_CAMS, G.FIX_CAMS, G.FIX_K, G.FIX_W, G.FIX_H, n_rays=n_rays, symmetric=True)
    f.requires_grad_(False)
    sym = [event_ms(ref2.step)[0] for _ in range(warmup + steps)][warmup:]
    f.requires_grad_(True)
    out["step_symmetric"] = round(statistics.median(sym), 4)
    return out


def kernels_alone(blk, dev, n, reps):
    f = blk[0]
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (torch.rand(n, 3, generator=gen, device=dev) - 0.5) * 3.0
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, device=dev), dim=-1)
    gs, gc = torch.randn(n, generator=gen, device=dev), torch.randn(n, 3, generator=gen, device=dev)
    gb, gcol = field_train.points_bwd(f, x, d, gs, gc)
    field_train.points_input_grad(f, x, d, gs, gc)
    ti, tb = [], []
    for _ in range(reps):                                         # alternated
        ti.append(event_ms(lambda: field_train.points_input_grad(f, x, d, gs, gc))[0])
        tb.append(event_ms(lambda: field_train.points_bwd(f, x, d, gs, gc, gb, gcol))[0])
    return {"points": n, "points_input_grad_ms": round(statistics.median(ti), 4), "points_bwd_ms": round(statistics.median(tb), 4)}


def accuracy(blk, iters, n_rays):
    gt = torch.eye(4, dtype=torch.float64)
    rows = []
    for deg in STARTS_DEG:
        start = start_pose(deg)
        pose, info = PR.refine_pose_photometric(blk, blk, start, G.FIX_CAMS, G.FIX_CAMS, G.FIX_K, G.FIX_W, G.FIX_H, iters=iters, n_rays=n_rays)
        r0, t0 = PR.pose_errors(start, gt)
        r1, t1 = PR.pose_errors(pose, gt)
        rows.append({"start_deg": deg, "start_t": 0.01 * deg, "start_rre_deg": r0, "start_rte": t0, "rre_deg": r1, "rte": t1, "iterations": iters,
                     "skipped": info["skipped"], "loss_first": info["loss"][0], "loss_last": info["loss"][-1], "mask_last": info["mask"][-1]})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200, help="iterations of the accuracy runs (refine_pose_photometric's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_refine_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photo_refine.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    blk = block(dev, args.res)
    res = {"device": torch.cuda.get_device_name(0), "grid": args.res, "rays": args.rays, "steps": args.steps, "warmup": args.warmup,
           "image": [G.FIX_W, G.FIX_H], "render_step_size": G.FIX_DT,
           "defaults_not_tuned": {"lr": 2e-3, "depth_weight": 0.1, "iters": 200, "n_rays": 4096, "opacity_threshold": PR.OPACITY_THRESHOLD}}
    res["ms_per_iteration"] = phases(blk, dev, args.rays, args.steps, args.warmup)
    res["kernels_alone"] = kernels_alone(blk, dev, 1 << 18, 10)
    res["accuracy"] = accuracy(blk, args.iters, args.rays)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
