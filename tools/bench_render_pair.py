#!/usr/bin/env python3
"""The fused two-block renderer (csrc/render_pair.hip) at the evaluator's frame size, beside the two one-block renders eval_nerf_regtr.py
--render_views makes for the same views: two generated 128^3 blocks (the thick shell of tools/bench_render.py, seeds 0 and 1), a relative pose
of 20 degrees about z and a translation of length 0.3, 12 look-at cameras at 800 x 800 (objaverse intrinsics) in the target frame,
render_step_size 0.005, white background.  The two paths alternate view by view after a warm-up; per path the median over the 12 views of
the device time per frame (events around the call, which reads the surviving-sample count back) and the surviving samples per second.
  pair       render_pair_image: one launch, both blocks in depth order, one image
  two_calls  render_image(target, view) + render_image(source, inv(P) @ view): two launches, two images that nothing composites
Writes one JSON object (--out, default profiles/render_pair_bench.json) and prints it.  Needs a GPU.
usage: python tools/bench_render_pair.py [--out PATH]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_pair_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_pair.py measures on the GPU; none found")
    blocks = [BR.make_block(seed=s) for s in (0, 1)]                      # source, target
    grids = [R.BlockGrid(AABB, occ.binary.to(DEV)) for _, occ in blocks]
    fields = [f for f, _ in blocks]
    a = math.radians(20.0)
    P = torch.eye(4)
    P[:3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    P[:3, 3] = torch.tensor([0.2, -0.2, 0.1])                              # |t| = 0.3
    Pinv = torch.linalg.inv(P)
    K, W, H = R.intrinsics("objaverse")
    cams = [BR.look_at((2.7 * math.cos(az) * math.cos(el), 2.7 * math.sin(az) * math.cos(el), 2.7 * math.sin(el)))
            for az, el in [(2 * math.pi * k / 6, el) for el in (0.35, -0.3) for k in range(6)]]
    dt, bk = 0.005, torch.ones(3, device=DEV)
    opts = dict(scene_aabb=AABB, render_step_size=dt)
    centers = [torch.tensor([0.0, -2.7, 0.5]), torch.tensor([2.7, 0.0, 0.5])]
    rays_t = [R.pixel_rays(c.to(DEV), K, W, H) for c in cams]
    rays_s = [R.pixel_rays((Pinv @ c).to(DEV), K, W, H) for c in cams]   # what --render_views renders the source block from

    def pair(i):
        return R.render_pair_image(fields[0], grids[0], fields[1], grids[1], rays_t[i], P, opts, opts, centers[0], centers[1], render_bkgd=bk)

    def two_calls(i):
        t = R.render_image(fields[1], grids[1], rays_t[i], AABB, render_step_size=dt, render_bkgd=bk)
        s = R.render_image(fields[0], grids[0], rays_s[i], AABB, render_step_size=dt, render_bkgd=bk)
        return t, s

    for i in range(2):                                                     # warm-up
        pair(i)
        two_calls(i)
    torch.cuda.synchronize()
    ms = {"pair": [], "two_calls": []}
    samples = {"pair": [], "two_calls": []}
    for i in range(len(cams)):
        out, t = _timed(lambda: pair(i))
        ms["pair"].append(t)
        samples["pair"].append(out[4])
        (ot, os_), t = _timed(lambda: two_calls(i))
        ms["two_calls"].append(t)
        samples["two_calls"].append(ot[3] + os_[3])
    res = {"bench": "render_pair", "blocks": "two 128^3 generated, shell 0.6-1.05", "pose": "20 deg about z, |t| = 0.3", "frames": len(cams),
           "width": W, "height": H, "render_step_size": dt}
    for k in ms:
        med = float(np.median(ms[k]))
        res[k] = {"ms_per_frame_median": round(med, 3), "ms_per_frame_min": round(min(ms[k]), 3), "ms_per_frame_max": round(max(ms[k]), 3),
                  "surviving_samples_per_frame": int(np.mean(samples[k])),
                  "surviving_samples_per_s": round(float(np.median([n / (t * 1e-3) for n, t in zip(samples[k], ms[k])])))}
    res["pair_over_two_calls"] = round(res["pair"]["ms_per_frame_median"] / res["two_calls"]["ms_per_frame_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=2)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
