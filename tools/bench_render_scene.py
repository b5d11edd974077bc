#!/usr/bin/env python3
"""The fused K-block renderer (csrc/render_scene.hip) at the evaluator's frame size, K = 2, 3, 4, beside the K one-block renders of the same
view and, at K = 2, beside the two-block kernel: generated 128^3 blocks (the thick shell of tools/bench_render.py, seeds 0..3), block poses of
20 degrees about z / x / y / (1,1,1) with |t| = 0.3 (the last block of a scene takes the rays as they are), 12 look-at cameras at 800 x 800
(objaverse intrinsics), render_step_size 0.005, white background.  The paths alternate view by view after a warm-up; per path the median over
the 12 views of the device time per frame (events around the call, which reads the surviving-sample count back) and the surviving samples
per second.
  scene      render_scene_image: one launch, K blocks in depth order, one image
  k_calls    K x render_image, each block from the view brought into its frame: K launches, K images that nothing composites
  pair       (K = 2) render_pair_image of the same two blocks: the same image, bit for bit
No target is set: the yardsticks are the existing kernels, measured in the same run.
Writes one JSON object (--out, default profiles/render_scene_bench.json) and prints it.  Needs a GPU.
usage: python tools/bench_render_scene.py [--out PATH]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dreg_nerf_amd import render as R  # noqa: E402
import bench_render as BR  # noqa: E402

DEV, AABB = BR.DEV, BR.AABB


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _pose(axis, deg, t):
    ax = torch.tensor(axis, dtype=torch.float64)
    ax = ax / ax.norm()
    a = math.radians(deg)
    Kx = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=torch.float64)
    P = torch.eye(4, dtype=torch.float64)
    P[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(a) * Kx + (1 - math.cos(a)) * (Kx @ Kx)
    P[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return P.float()


def _stats(ms, samples):
    med = float(np.median(ms))
    return {"ms_per_frame_median": round(med, 3), "ms_per_frame_min": round(min(ms), 3), "ms_per_frame_max": round(max(ms), 3),
            "surviving_samples_per_frame": int(np.mean(samples)),
            "surviving_samples_per_s": round(float(np.median([n / (t * 1e-3) for n, t in zip(samples, ms)])))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_scene_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_scene.py measures on the GPU; none found")
    made = [BR.make_block(seed=s) for s in range(4)]
    grids = [R.BlockGrid(AABB, occ.binary.to(DEV)) for _, occ in made]
    fields = [f for f, _ in made]
    poses = [_pose((0, 0, 1), 20.0, (0.2, -0.2, 0.1)), _pose((1, 0, 0), 20.0, (-0.1, 0.2, 0.2)), _pose((0, 1, 0), 20.0, (0.2, 0.1, -0.2)),
             _pose((1, 1, 1), 20.0, (-0.2, -0.1, -0.2))]                    # |t| = 0.3 each
    centers = [torch.tensor([0.0, -2.7, 0.5]), torch.tensor([2.7, 0.0, 0.5]), torch.tensor([0.0, 2.7, 0.5]), torch.tensor([-2.7, 0.0, 0.5])]
    Kc, W, H = R.intrinsics("objaverse")
    cams = [BR.look_at((2.7 * math.cos(az) * math.cos(el), 2.7 * math.sin(az) * math.cos(el), 2.7 * math.sin(el)))
            for az, el in [(2 * math.pi * k / 6, el) for el in (0.35, -0.3) for k in range(6)]]
    dt, bk = 0.005, torch.ones(3, device=DEV)
    opts = dict(scene_aabb=AABB, render_step_size=dt)
    rays = [R.pixel_rays(c.to(DEV), Kc, W, H) for c in cams]
    res = {"bench": "render_scene", "blocks": "128^3 generated, shell 0.6-1.05, seeds 0..3", "poses": "20 deg about z / x / y / (1,1,1), |t| = 0.3; last block: rays as given",
           "frames": len(cams), "width": W, "height": H, "render_step_size": dt}
    for n in (2, 3, 4):
        P = poses[:n - 1] + [None]
        blocks = [(fields[b], grids[b], opts, centers[b], P[b]) for b in range(n)]
        rays_b = [[r if P[b] is None else R.rays_to_block(r, P[b]) for r in rays] for b in range(n)]   # what K one-block calls march

        def scene(i):
            return R.render_scene_image(blocks, rays[i], render_bkgd=bk)

        def k_calls(i):
            return [R.render_image(fields[b], grids[b], rays_b[b][i], AABB, render_step_size=dt, render_bkgd=bk) for b in range(n)]

        def pair(i):
            return R.render_pair_image(fields[0], grids[0], fields[1], grids[1], rays[i], P[0], opts, opts, centers[0], centers[1], render_bkgd=bk)

        paths = {"scene": (scene, lambda o: o[4]), "k_calls": (k_calls, lambda o: sum(x[3] for x in o))}
        if n == 2:
            paths["pair"] = (pair, lambda o: o[4])
        for i in range(2):                                                 # warm-up
            for fn, _ in paths.values():
                fn(i)
        torch.cuda.synchronize()
        ms, samples = {k: [] for k in paths}, {k: [] for k in paths}
        for i in range(len(cams)):
            for k, (fn, count) in paths.items():
                out, t = _timed(lambda: fn(i))
                ms[k].append(t)
                samples[k].append(count(out))
        row = {k: _stats(ms[k], samples[k]) for k in paths}
        row["scene_over_k_calls"] = round(row["scene"]["ms_per_frame_median"] / row["k_calls"]["ms_per_frame_median"], 3)
        if n == 2:
            row["scene_over_pair"] = round(row["scene"]["ms_per_frame_median"] / row["pair"]["ms_per_frame_median"], 3)
        res[f"K{n}"] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
