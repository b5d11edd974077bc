#!/usr/bin/env python3
"""Step time of the 4-pair 128^3 bf16 training step (bench.py's workload) with the opt-in pose loss off, on the last decoder layer and on all six,
alternated in one process (TrainStep.pose_loss_weight / pose_loss_layers switched between timed windows of the same model and optimizer).
usage: python tools/bench_pose_loss.py [--steps K] [--rounds N] [--res R] [--pairs P] [--out FILE.json]
Under `rocprofv3 --kernel-trace --stats -- python tools/bench_pose_loss.py --steps 3 --rounds 1` it gives the kernel table of the three settings."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreg_nerf_amd import synth  # noqa: E402
from dreg_nerf_amd.regtr import NeRFRegTr  # noqa: E402
from dreg_nerf_amd.train_step import TrainStep  # noqa: E402

SETTINGS = {"off": (0.0, "last"), "last": (1.0, "last"), "all": (1.0, "all")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per setting (the settings alternate)")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(3407)
    model = NeRFRegTr(precision="bf16").to(dev).train()
    ts = TrainStep(model)
    pose = synth.fixed_pose()
    batch = []
    for i in range(args.pairs):
        d = synth.shell_pair(args.res, 1 + 2 * i, 2 + 2 * i, pose=pose)
        batch.append({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()})
    times = {k: [] for k in SETTINGS}
    losses = {}
    for name, (w, layers) in SETTINGS.items():      # warm-up: every setting's shapes and launches
        ts.pose_loss_weight, ts.pose_loss_layers = w, layers
        for _ in range(2):
            ts.step(batch)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (w, layers) in SETTINGS.items():
            ts.pose_loss_weight, ts.pose_loss_layers = w, layers
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                out = ts.step(batch)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
            losses[name] = {k: float(v) for k, v in out["losses"].items()}
    rec = {"res": args.res, "pairs": args.pairs, "steps_per_window": args.steps, "rounds": args.rounds,
           "ms_per_step_median": {k: statistics.median(v) for k, v in times.items()},
           "ms_per_step_windows": times, "last_losses": losses}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
