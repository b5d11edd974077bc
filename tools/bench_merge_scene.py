"""Field distillation of a registered scene on one MI355X: generated 128^3 blocks, K = 2 and 4, 2^16 points per step.  Reports
ms per step split into sampler, teacher (scene_radiance), student forward (field_points), backward as a caller sees it, Adam and occupancy update
(amortised over its 16 steps), the measured whole step, and the kernel's own share: one dreg_ngp_points_bwd call on preallocated buffers, and the
same call with zero upstream gradients (workspace memset + empty launch + slab reduce), whose difference is the chain launch.  Medians of --steps
steps after --warmup, event pairs.  Beside that, in the same call: dreg_ngp_points_bwd alone at 2^18 points against dreg_ngp_render_bwd at about
2^18 samples on tools/bench_train_ngp.py's setup.

    python tools/bench_merge_scene.py [--steps 50 --warmup 20 --out profiles/merge_scene_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dreg_nerf_amd import field_train, ngp, ngp_train, scene_merge  # noqa: E402
from dreg_nerf_amd.scene_field import SceneField  # noqa: E402

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]


def _block(dev, seed):
    torch.manual_seed(seed)
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params[3072:].uniform_(-1.0, 1.0)
    f = f.to(dev).eval()
    g = ngp.OccupancyGrid(AABB, 128).to(dev)
    c = (torch.stack(torch.meshgrid(*[torch.arange(128)] * 3, indexing="ij"), -1).float() + 0.5) / 128 * 3.0 - 1.5
    g._binary = (c.norm(dim=-1) < 0.8).to(dev)
    return f, g


def _pose(k):
    P = torch.eye(4, dtype=torch.float64)
    P[:3, 3] = torch.tensor([0.3 * k, -0.2 * k, 0.1 * k], dtype=torch.float64)
    return P


def _steps(dev, K, steps, warmup, points):
    """Medians over the timed steps, ms.  `step` is ONE event pair around the whole step, sampler included: it is measured, not a sum of the
    columns.  `backward` is what a caller sees between the loss and the optimiser (torch's loss launches, autograd, two zero-filled gradient
    buffers, dreg_ngp_points_bwd); the kernel's own share is timed on the same points right after the step, on preallocated buffers:
    `points_bwd_call` = one dreg_ngp_points_bwd (workspace memset, the chain launch, the slab reduce), `memset_reduce` = the same call with
    all-zero upstream gradients (every pass is skipped: the memset, an empty launch and the reduce remain), so the chain launch itself is their
    difference."""
    blocks = [_block(dev, 10 + k) for k in range(K)]
    sf = SceneField([(f, g, [0.0, 0.0, 3.0], None if k == 0 else _pose(k)) for k, (f, g) in enumerate(blocks)])
    torch.manual_seed(0)
    dist = scene_merge.SceneDistiller(sf, n_points=points, max_iterations=20000)
    dist.field.train()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    names = ("sample", "teacher", "forward", "backward", "adam", "points_bwd_call", "memset_reduce")
    rows = {k: [] for k in names + ("step",)}
    gb = torch.zeros(dist.field.mlp_base.params.numel(), device=dev)
    gc = torch.zeros(7168, device=dev)
    zs, zc = torch.zeros(points, device=dev), torch.zeros(points, 3, device=dev)
    for it in range(warmup + steps):
        e = [ev() for _ in range(8)]
        e[0].record()
        x, d = dist.sample()
        e[1].record()
        st, ct = scene_merge.scene_radiance(sf, x, d)
        e[2].record()
        ss, cs = field_train.field_points(dist.field, x, d)
        e[3].record()
        loss = scene_merge.distill_loss(ss, cs, st, ct)
        dist.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        e[4].record()
        dist.optimizer.step()
        dist.scheduler.step()
        e[5].record()
        field_train.points_bwd(dist.field, x, d, st, ct, gb, gc)      # (any non-zero upstream gradients of the step's shapes: the teacher's values)
        e[6].record()
        field_train.points_bwd(dist.field, x, d, zs, zc, gb, gc)
        e[7].record()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(names):
                rows[name].append(e[k].elapsed_time(e[k + 1]))
            rows["step"].append(e[0].elapsed_time(e[5]))
    dist.grid.train()
    occ = []
    for _ in range(5):
        a, b = ev(), ev()
        a.record()
        dist.grid._update(1000, dist.occ_eval_fn)
        b.record()
        torch.cuda.synchronize()
        occ.append(a.elapsed_time(b))
    out = {k: round(statistics.median(v), 3) for k, v in rows.items()}
    out["chain_launch"] = round(out["points_bwd_call"] - out["memset_reduce"], 3)
    out["occupancy_amortised"] = round(statistics.median(occ) / 16, 3)
    return out


def _points_bwd_alone(dev, n, reps):
    f, _ = _block(dev, 3)
    f.train()
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (torch.rand(n, 3, generator=gen, device=dev) - 0.5) * 3.0
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen, device=dev), dim=-1)
    gs, gc = torch.randn(n, generator=gen, device=dev), torch.randn(n, 3, generator=gen, device=dev)
    gb, gcol = field_train.points_bwd(f, x, d, gs, gc)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        field_train.points_bwd(f, x, d, gs, gc, gb, gcol)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 3)


def _render_bwd_alone(dev, reps):
    import bench_train_ngp as BT
    torch.manual_seed(0)
    field = ngp.NGPradianceField(AABB).to(dev)
    grid = ngp.OccupancyGrid(AABB, 128).to(dev)
    c = (torch.stack(torch.meshgrid(*[torch.arange(128)] * 3, indexing="ij"), -1).float() + 0.5) / 128 * 3.0 - 1.5
    grid._binary = (c.norm(dim=-1) < 0.8).to(dev)
    views = BT._Views(dev, n=8)
    field.train()
    dt = ngp_train.render_step_size_of(AABB)
    num_rays, n = ngp_train.TARGET_SAMPLES // 1024, 0
    for _ in range(6):                                    # the trainer's own rule towards 2^18 surviving samples
        rs, _ = views.sample(num_rays)
        with torch.no_grad():
            n = ngp_train.render_image_train(field, grid, rs, AABB, dt, torch.ones(3))[3]
        num_rays = max(1, ngp_train.next_num_rays(num_rays, max(n, 1)))
    ts, ns = [], []
    for _ in range(reps):
        rs, _ = views.sample(num_rays)
        rgb, _, _, n = ngp_train.render_image_train(field, grid, rs, AABB, dt, torch.ones(3))
        g = torch.randn_like(rgb)
        field.mlp_base.params.grad = field.color_mlp.params.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rgb.backward(g)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
        ns.append(n)
    return round(statistics.median(ts), 3), int(statistics.median(ns))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_scene_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"metric": "merge_scene_ms_per_step", "points": args.points, "steps": args.steps, "warmup": args.warmup, "grid": 128}
    for K in (2, 4):
        res[f"K{K}"] = _steps(dev, K, args.steps, args.warmup, args.points)
    res["points_bwd_ms_at_2^18_points"] = _points_bwd_alone(dev, 1 << 18, 10)
    ms, n = _render_bwd_alone(dev, 5)
    res["render_bwd_ms"], res["render_bwd_samples"] = ms, n
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump(res, fp, indent=1)


if __name__ == "__main__":
    main()
