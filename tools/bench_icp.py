#!/usr/bin/env python3
"""Point-to-plane ICP refinement on the test solid at 128^3 (tests/icp_cases.py: a box with a step, surface cells with exact axis normals): the source
points are the target points moved by a known pose, the run starts from the identity.

  accuracy   initial errors of 0.5 / 1 / 2 / 3 / 5 degrees with |t| = 1 % of the angle in degrees, target normals exact and by PCA
             (icp.block_normals without a field): final RRE / RTE, iterations, fitness and status per start
  time       ms per refinement (--iters iterations, no early freeze: tolerances 0) from hipEvent pairs after warm-up, the fused call
             (dreg_icp_refine: 2 launches per iteration, pose on the device) and a torch-composed loop on the same inputs (chunked cdist argmin
             plus the normal equations and a 6x6 solve in torch, pose on the device too), alternated, median of --rounds.  The composed loop is
             the baseline, not code under test.

Writes one JSON object (--out, default profiles/icp_bench.json).  Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_cases as IC  # noqa: E402
import icp_restatement as IR  # noqa: E402
from dreg_nerf_amd import icp  # noqa: E402

STARTS_DEG = (0.5, 1.0, 2.0, 3.0, 5.0)
MAX_DIST = 0.05


def composed_refine(src, tgt, nrm, pose, max_dist, iters, chunk=4096):
    """The same iteration in torch ops: nearest neighbour by chunked cdist, gate, residuals, J^T J and J^T e, solve, exponential map.  fp32 points,
    fp64 normal equations, everything on the device, no host synchronisation."""
    R, t = pose[:3, :3].clone(), pose[:3, 3].clone()
    for _ in range(iters):
        q = src @ R.float().T + t.float()
        best = torch.cat([torch.cdist(q[a:a + chunk], tgt).argmin(dim=1) for a in range(0, q.shape[0], chunk)])
        r = q - tgt[best]
        n = nrm[best]
        ok = ((r * r).sum(dim=1) <= max_dist * max_dist).double()[:, None]
        e = (n * r).sum(dim=1, keepdim=True).double()
        J = torch.cat([torch.cross(q, n, dim=1), n], dim=1).double() * ok
        xi = -torch.linalg.solve(J.T @ J, J.T @ (e * ok))[:, 0]
        w, v = xi[:3], xi[3:]
        th = w.norm().clamp_min(1e-300)
        K = torch.zeros(3, 3, dtype=torch.float64, device=src.device)
        K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
        E = torch.eye(3, dtype=torch.float64, device=src.device) + torch.sin(th) / th * K + (1 - torch.cos(th)) / (th * th) * (K @ K)
        R, t = E @ R, E @ t + v
    out = torch.eye(4, dtype=torch.float64, device=src.device)
    out[:3, :3], out[:3, 3] = R, t
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_icp.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    pts, nrm = IC.test_solid(args.res)
    tgt = torch.from_numpy(pts).to(dev)
    normals = {"exact": torch.from_numpy(nrm).to(dev), "pca": icp.block_normals(tgt)}
    cell = icp.default_cell(MAX_DIST)
    index = {k: icp.TargetIndex(tgt, v, cell) for k, v in normals.items()}
    tdir = np.array([0.5, -0.7, 0.4]) / np.linalg.norm([0.5, -0.7, 0.4])
    accuracy = {k: [] for k in normals}
    srcs = {}
    for deg in STARTS_DEG:
        R, t = IC.rotation((0.3, -0.5, 0.8), deg), 0.01 * deg * tdir
        src = torch.from_numpy(((pts.astype(np.float64) - t) @ R).astype(np.float32)).to(dev)
        srcs[deg] = src
        for k in normals:
            pose, info = icp.refine_pose(src, index[k], torch.eye(4), max_dist=MAX_DIST, iters=args.iters)
            p = pose.cpu().numpy()
            accuracy[k].append({"start_deg": deg, "start_t": 0.01 * deg, "rre_deg": IR.rre_deg(p[:3, :3], R), "rte": IR.rte(p[:3, 3], t),
                                "iterations": info["iterations"], "status": info["status"], "fitness": info["fitness"], "plane_rmse": info["plane_rmse"]})
    # time: the 2 degree start, exact normals, every iteration runs (tolerances 0: no freeze)
    src, ix = srcs[2.0], index["exact"]
    eye = torch.eye(4, dtype=torch.float64, device=dev)
    paths = {"fused": lambda: fused(src, ix, args.iters),
             "composed": lambda: composed_refine(src, tgt, normals["exact"], eye, MAX_DIST, args.iters)}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.rounds):                                  # alternated: drift of the box hits both paths alike
        for k, fn in paths.items():
            times[k].append(event_ms(fn))
    a, b = fused(src, ix, args.iters), composed_refine(src, tgt, normals["exact"], eye, MAX_DIST, args.iters)
    res = {"res": args.res, "points": int(tgt.shape[0]), "max_dist": MAX_DIST, "cell": ix.cell, "grid": list(ix.dims), "iters": args.iters, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "accuracy": accuracy,
           "ms_per_refinement": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
           "fused_vs_composed_pose_max_abs_diff": float((a - b).abs().max())}
    med = {k: v["median"] for k, v in res["ms_per_refinement"].items()}
    res["ms_per_iteration"] = {k: v / args.iters for k, v in med.items()}
    res["speedup"] = med["composed"] / med["fused"]
    assert all(math.isfinite(v) for v in med.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def fused(src, index, iters):
    """The fused call alone (pose upload, launches), no readback of the stats table."""
    pose12 = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=src.device)
    icp.refine_launch(src, index, pose12, MAX_DIST, iters, 0.0, 0.0)
    out = torch.eye(4, dtype=torch.float64, device=src.device)
    out[:3, :3], out[:3, 3] = pose12[:9].reshape(3, 3), pose12[9:]
    return out


if __name__ == "__main__":
    main()
