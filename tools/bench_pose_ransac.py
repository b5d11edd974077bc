#!/usr/bin/env python3
"""Robust pose from correspondences on the two-mode case (tests/pose_ransac_cases.py): N correspondences drawn from the ICP test solid at 64^3, a
share of 55 % following a 25 degree motion and the rest the same motion after a further 40 degree turn about z, noise 0.005 on the matches,
H random triplets.

  accuracy   RRE / RTE of the plain weighted Kabsch solve, of the minimal pose and after the three consensus refits, inlier counts
  time       ms per scoring of all H hypotheses (score + select; the refits are the existing Kabsch kernel) from hipEvent pairs after warm-up:
             the fused call (dreg_pose_ransac) against a torch-composed score on the same triplets (triad in batched torch ops, then
             |R a + t - b|^2 <= thresh^2 counted in chunks of hypotheses so that the [chunk, N, 3] temporary stays below 64 MB, argmax),
             alternated, median of --rounds.  The composed score is the baseline, not code under test; no speed target is set.

Writes one JSON object (--out, default profiles/pose_ransac_bench.json).  Needs a GPU."""
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
import pose_ransac_cases as PC  # noqa: E402
from dreg_nerf_amd import attn_ops, pose_ransac  # noqa: E402

THRESH = 0.02


def case(n, seed=0, minority=0.45, sigma=0.005):
    pts, _ = IC.test_solid(64)
    rng = np.random.default_rng(seed)
    pts = pts[rng.permutation(len(pts))[:n]].astype(np.float64)
    Rz = IC.rotation((0.0, 0.0, 1.0), 40.0)
    minor = rng.permutation(n) < int(round(minority * n))
    b = np.where(minor[:, None], pts @ (PC.TWO_MODE_R1 @ Rz).T + PC.TWO_MODE_T1, pts @ PC.TWO_MODE_R1.T + PC.TWO_MODE_T1)
    b = b + rng.normal(scale=sigma, size=b.shape)
    return pts.astype(np.float32), b.astype(np.float32)


def composed_score(a, b, trip, thresh, eps_area=1e-4, chunk_bytes=64 << 20):
    """The same rule in torch ops, everything on the device: (best index, best count, pose [12])."""
    t = trip.long()

    def frame(p):
        e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
        n = torch.cross(e1, e2, dim=1)
        l1, l2, ln = (e1 * e1).sum(1), (e2 * e2).sum(1), (n * n).sum(1)
        u1, u3 = e1 / l1.sqrt()[:, None], n / ln.sqrt()[:, None]
        return torch.stack([u1, torch.cross(u3, u1, dim=1), u3], dim=1), ln > eps_area * l1 * l2

    U, oka = frame(a)
    V, okb = frame(b)
    valid = oka & okb & (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])
    R = V.transpose(1, 2) @ U
    tr = b[t[:, 0]] - (R @ a[t[:, 0]][:, :, None])[:, :, 0]
    chunk = max(1, chunk_bytes // (a.shape[0] * 12))
    counts = []
    for s in range(0, t.shape[0], chunk):
        q = a[None] @ R[s:s + chunk].transpose(1, 2) + tr[s:s + chunk, None]
        counts.append((((q - b[None]) ** 2).sum(-1) <= thresh * thresh).sum(1))
    counts = torch.where(valid, torch.cat(counts), torch.full_like(counts[0][:1], -1))
    h = counts.argmax()
    return h, counts[h], torch.cat([R[h].reshape(9), tr[h]])


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--hyps", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_ransac_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_ransac.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    a_np, b_np = case(args.n)
    a, b = torch.from_numpy(a_np).to(dev), torch.from_numpy(b_np).to(dev)
    trip = pose_ransac.draw_triplets(args.n, args.hyps, 0, dev)
    R, t = PC.TWO_MODE_R1, PC.TWO_MODE_T1

    def err(p34):
        p = p34.detach().cpu().double().numpy()
        return dict(zip(("rre_deg", "rte"), PC.pose_errors(np.concatenate([p[:, :3].reshape(9), p[:, 3]]), R, t)))

    pose, info = pose_ransac.estimate_pose(a, b, thresh=THRESH, triplets=trip)
    plain = attn_ops.weighted_kabsch(a[None], b[None], torch.ones(1, args.n, device=dev))[0]
    accuracy = {"weighted_kabsch": err(plain), "minimal": dict(err(info["minimal_pose"]), inliers=info["minimal_inliers"], index=info["best_index"]),
                "after_refits": dict(err(pose), inliers=info["inliers"], round_inliers=info["round_inliers"], round_used=info["round_used"])}
    paths = {"fused": lambda: pose_ransac.ransac_launch(a, b, trip, THRESH), "composed": lambda: composed_score(a, b, trip, THRESH)}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(args.rounds):                                  # alternated: drift of the box hits both paths alike
        for k, fn in paths.items():
            times[k].append(event_ms(fn))
    f, c = paths["fused"](), paths["composed"]()
    torch.cuda.synchronize()
    res = {"n": args.n, "hyps": args.hyps, "thresh": THRESH, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "accuracy": accuracy,
           "ms_per_call": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
           "fused_best": f["best"].tolist(), "composed_best": [int(c[0]), int(c[1])],
           "note": "the composed score rounds differently (matrix products, no fixed operation order): its best index and count may differ by a few near-threshold points"}
    med = {k: v["median"] for k, v in res["ms_per_call"].items()}
    res["speedup"] = med["composed"] / med["fused"]
    assert all(math.isfinite(v) for v in med.values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
