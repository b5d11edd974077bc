"""NeRF block training step at the reference's operating point (one MI355X): 800 x 800 views, 2^18 rendered samples per step, a 128^3
occupancy grid, tcnn's initial field.  Reports ms per step split into occupancy update (amortised over its 16 steps), training forward,
backward (loss + dreg_ngp_render_bwd), fused Adam and host, with surviving samples/s and the hash-table scatter's added bytes per second of the
backward launch (an upper-bound time: the launch also re-marches and runs both networks).

    python tools/bench_train_ngp.py --steps 50 --warmup 20 [--backward samples] [--out profiles/train_ngp_bench.json]

--backward samples times the sample-list path (dreg_ngp_render_train_samples, the sort, dreg_ngp_samples_grad, dreg_ngp_points_bwd)
instead of the ray backward; the figures keep their names (forward_ms then includes the list write and the sort).
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dreg_nerf_amd import ngp, ngp_train, render  # noqa: E402


class _Views:
    """Random pixels of 32 800 x 800 cameras on a sphere of radius 4 around a ball of radius 0.8 (white background, grey ball)."""

    def __init__(self, dev, n=32):
        K, W, H = render.intrinsics("objaverse")
        g = torch.Generator().manual_seed(0)
        rays = []
        for _ in range(n):
            z = float(torch.rand(1, generator=g)) * 1.6 - 0.8
            phi = float(torch.rand(1, generator=g)) * 2 * math.pi
            pos = torch.tensor([math.sqrt(1 - z * z) * math.cos(phi), math.sqrt(1 - z * z) * math.sin(phi), z]) * 4.0
            fwd = -pos / pos.norm()
            right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]))
            right = right / right.norm()
            up = torch.linalg.cross(right, fwd)
            c2w = torch.eye(4)
            c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, -fwd, pos
            r = render.pixel_rays(c2w.to(dev), K, W, H)
            rays.append((r.origins.reshape(-1, 3), r.viewdirs.reshape(-1, 3)))
        self.o = torch.cat([r[0] for r in rays])
        self.d = torch.cat([r[1] for r in rays])
        self.dev = dev

    def sample(self, n):
        i = torch.randint(0, self.o.shape[0], (n,), device=self.dev)
        return render.Rays(self.o[i].contiguous(), self.d[i].contiguous()), torch.full((n, 3), 0.5, device=self.dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--backward", choices=["rays", "samples"], default="rays")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    aabb = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    field = ngp.NGPradianceField(aabb).to(dev)
    grid = ngp.OccupancyGrid(aabb, 128).to(dev)
    c = (torch.stack(torch.meshgrid(*[torch.arange(128)] * 3, indexing="ij"), -1).float() + 0.5) / 128 * 3.0 - 1.5
    grid._binary = (c.norm(dim=-1) < 0.8).to(dev)
    tr = ngp_train.NGPTrainer(field, grid, _Views(dev), aabb, 20000)
    tr.grid.every_n_step = lambda *a, **k: None         # timed on its own below (warm-up would otherwise reset the ball)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    tot = {"fwd": 0.0, "bwd": 0.0, "adam": 0.0, "step": 0.0}
    samples = rays = 0
    it = 0
    for k in range(args.warmup + args.steps):
        timed = k >= args.warmup
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e = [ev() for _ in range(4)]
        e[0].record()
        rs, px = tr.data.sample(tr.num_rays)
        if args.backward == "samples":
            rgb, opac, _, n = ngp_train.render_image_train(field, grid, rs, aabb, tr.render_step_size, tr.bkgd, backward="samples")
        else:
            rgb, opac, _, n = ngp_train.render_image_train(field, grid, rs, aabb, tr.render_step_size, tr.bkgd)
        e[1].record()
        alive = opac.squeeze(-1) > 0
        loss = torch.nn.functional.smooth_l1_loss(rgb[alive], px[alive])
        tr.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        e[2].record()
        tr.optimizer.step()
        tr.scheduler.step()
        e[3].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if timed:
            tot["fwd"] += e[0].elapsed_time(e[1])
            tot["bwd"] += e[1].elapsed_time(e[2])
            tot["adam"] += e[2].elapsed_time(e[3])
            tot["step"] += (t1 - t0) * 1e3
            samples += n
            rays += len(px)
        tr.num_rays = max(1, ngp_train.next_num_rays(len(px), n))
        it += 1
    # occupancy update after warm-up (steps >= 256: a quarter uniform + a quarter occupied cells), amortised over 16 steps
    g2 = ngp.OccupancyGrid(aabb, 128).to(dev)
    g2._binary = grid._binary.clone()
    g2.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        g2._update(1000, tr.occ_eval_fn)
    torch.cuda.synchronize()
    occ_ms = (time.perf_counter() - t0) * 1e3 / 5
    S = args.steps
    fwd, bwd, adam, step = tot["fwd"] / S, tot["bwd"] / S, tot["adam"] / S, tot["step"] / S
    res = {"metric": "ngp_train_ms_per_step", "value": round(step + occ_ms / 16, 3), "occupancy_amortised_ms": round(occ_ms / 16, 3),
           "occupancy_update_ms": round(occ_ms, 3), "forward_ms": round(fwd, 3), "backward_ms": round(bwd, 3), "adam_ms": round(adam, 3),
           "host_ms": round(step - fwd - bwd - adam, 3), "surviving_samples_per_step": samples // S, "rays_per_step": rays // S,
           "surviving_samples_per_s_fwd": round(samples / S / (fwd * 1e-3)), "surviving_samples_per_s_bwd": round(samples / S / (bwd * 1e-3)),
           "hash_scatter_TBps_over_backward": round(samples / S * 1024 / (bwd * 1e-3) / 1e12, 4), "steps": S, "warmup": args.warmup,
           "views": "800x800", "grid": 128, "target_samples": ngp_train.TARGET_SAMPLES, "backward": args.backward}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(res, fp, indent=1)


if __name__ == "__main__":
    main()
