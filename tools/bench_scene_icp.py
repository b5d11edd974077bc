#!/usr/bin/env python3
"""Joint K-block point-to-plane ICP on partial views of the test solid at 128^3 (tests/scene_icp_cases.py: three and four
overlapping views, each under a known motion; every run starts from the identity, so the start error is the whole motion).

Per K in (3, 4) and per start of 0.5 / 1 / 2 / 3 / 5 degrees with |t| = 1 % of the angle in degrees:
  joint      scene_icp.refine_poses: one call, all K (K - 1) ordered pairs in every iteration — worst RRE / RTE over the blocks, iterations, status,
             fitness;
  pairwise   the K (K - 1) icp.refine_pose calls (each from the identity) followed by pose_graph.synchronize: the same errors.
Time: ms per refinement at the 2 degree start (--iters iterations, no early freeze: tolerances 0) from hipEvent pairs after warm-up, the joint
launch sequence against the K (K - 1) pair launch sequences (no readback in either; the synchronisation on the host is not timed), alternated,
median of --rounds.

Writes one JSON object (--out, default profiles/scene_icp_bench.json).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_icp_cases as SC  # noqa: E402
import scene_icp_restatement as SR  # noqa: E402
from dreg_nerf_amd import icp, pose_graph, scene_icp  # noqa: E402

STARTS_DEG = (0.5, 1.0, 2.0, 3.0, 5.0)
MAX_DIST = 0.05


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def scene(K, res, deg, dev):
    points, normals, G_true = SC.view_case(K, res, deg_len=(deg, 0.01 * deg))
    pts = [torch.from_numpy(p).to(dev) for p in points]
    idx = [icp.TargetIndex(p, torch.from_numpy(n).to(dev), icp.default_cell(MAX_DIST)) for p, n in zip(pts, normals)]
    return pts, idx, G_true


def pairwise(pts, idx, iters):
    """K (K - 1) pair refinements from the identity, then the synchronisation: G12 [K,12] and the pairs' statuses."""
    K = len(pts)
    edges, statuses = [], []
    for i in range(K):
        for j in range(K):
            if i != j:
                pose, info = icp.refine_pose(pts[i], idx[j], torch.eye(4), max_dist=MAX_DIST, iters=iters)
                edges.append((i, j, pose.cpu().numpy(), 1.0))
                statuses.append(info["status"])
    G, _ = pose_graph.synchronize(K, edges, anchor=0)
    return SR.poses12_of(np.asarray(G)), statuses


def joint_launch(pts, idx, iters):
    poses = torch.tensor(SC.identity_poses(len(pts)), dtype=torch.float64, device=pts[0].device)
    return scene_icp.refine_launch(pts, idx, poses, MAX_DIST, iters, 0.0, 0.0)


def pair_launches(pts, idx, iters):
    keep = []
    for i in range(len(pts)):
        for j in range(len(pts)):
            if i != j:
                pose12 = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=pts[0].device)
                keep.append(icp.refine_launch(pts[i], idx[j], pose12, MAX_DIST, iters, 0.0, 0.0))
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_icp_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_icp.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    res = {"res": args.res, "max_dist": MAX_DIST, "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "scenes": {}}
    for K in (3, 4):
        rows = []
        for deg in STARTS_DEG:
            pts, idx, G_true = scene(K, args.res, deg, dev)
            G, info = scene_icp.refine_poses(pts, idx, torch.eye(4).repeat(K, 1, 1), max_dist=MAX_DIST, iters=args.iters)
            rre, rte = SC.worst_errors(SR.poses12_of(G.cpu().numpy()), G_true)
            Gp, statuses = pairwise(pts, idx, args.iters)
            rre_p, rte_p = SC.worst_errors(Gp, G_true)
            rows.append({"start_deg": deg, "start_t": 0.01 * deg,
                         "joint": {"rre_deg": rre, "rte": rte, "iterations": info["iterations"], "status": info["status"], "fitness": info["fitness"]},
                         "pairwise": {"rre_deg": rre_p, "rte": rte_p, "statuses": statuses}})
        pts, idx, _ = scene(K, args.res, 2.0, dev)
        paths = {"joint": lambda: joint_launch(pts, idx, args.iters), "pairwise": lambda: pair_launches(pts, idx, args.iters)}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(args.rounds):                              # alternated: drift of the box hits both paths alike
            for k, fn in paths.items():
                times[k].append(event_ms(fn))
        ms = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        res["scenes"][str(K)] = {"points": [int(p.shape[0]) for p in pts], "accuracy": rows, "ms_per_refinement": ms,
                                 "launches": {"joint": 1 + 2 * args.iters, "pairwise": 2 * args.iters * K * (K - 1)},
                                 "speedup": ms["pairwise"]["median"] / ms["joint"]["median"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
