#!/usr/bin/env python3
"""The fused volume renderer (csrc/render.hip) at the evaluator's frame size: a generated 128^3 block (the _make_block recipe of
tests/test_hip_chain_config5.py with a denser shell), 12 look-at cameras at 800 x 800 (objaverse intrinsics), render_step_size 0.005, white
background.  After warm-up: ms per frame, rays/s and surviving samples/s of the fused kernel; then the same frames through a torch-composed
path with the reference's structure on this tree's kernels (host-side marching restatement, query_density / query_rgb in test_chunk_size
chunks, compositing in torch) — its time and the agreement between the two.  Prints one JSON line.
usage: python tools/bench_render.py [--frames-torch N]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreg_nerf_amd import ngp  # noqa: E402
from dreg_nerf_amd import render as R  # noqa: E402

DEV = torch.device("cuda", 0)
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]


def make_block(res=128, shell=(0.6, 1.05), seed=0):
    g = torch.Generator().manual_seed(seed)
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params[:3072] = torch.randn(3072, generator=g) * 1.0
        f.mlp_base.params[3072:] = torch.randn(f.mlp_base.params.numel() - 3072, generator=g)
        f.color_mlp.params.copy_(torch.randn(7168, generator=g) * 0.2)
    c = (torch.arange(res, dtype=torch.float32) + 0.5) / res * 3 - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    rad = torch.stack([X, Y, Z], -1).norm(dim=-1)
    occ = ngp.OccupancyGrid(AABB, res)
    occ._binary.copy_((rad > shell[0]) & (rad < shell[1]))
    return f.to(DEV).eval(), occ


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    eye, target, up = torch.tensor(eye), torch.tensor(target), torch.tensor(up)
    back = torch.nn.functional.normalize(eye - target, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(up, back), dim=0)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, torch.linalg.cross(back, right), back, eye
    return c2w


@torch.no_grad()
def torch_composed(field, occ, rays, dt, bkgd, chunk=8192, eps=1e-4):
    """render_image's structure (ray_marching then rendering, per chunk) as torch ops around query_density / query_rgb."""
    o_all, d_all = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    binary = occ.binary.to(DEV)
    res = torch.tensor(binary.shape, device=DEV, dtype=torch.float32)
    hi_idx = torch.tensor(binary.shape, device=DEV) - 1
    roi = torch.tensor(AABB, device=DEV)
    out_rgb, out_op, out_dep, total = [], [], [], 0
    for i in range(0, o_all.shape[0], chunk):
        o, d = o_all[i:i + chunk], d_all[i:i + chunk]
        t0, t1 = (roi[:3] - o) / d, (roi[3:] - o) / d
        near, far = torch.minimum(t0, t1).max(-1).values, torch.maximum(t0, t1).min(-1).values
        hit = (near <= far) & (far > 0)
        tmin = near.clamp(min=0)
        span = torch.where(hit, far - tmin, torch.zeros_like(tmin))
        S = int(torch.ceil((span / dt).max()).item()) + 1
        tm = tmin[:, None] + (torch.arange(S, device=DEV, dtype=torch.float32)[None] + 0.5) * dt
        valid = (tm < far[:, None]) & hit[:, None]
        x = o[:, None] + tm[..., None] * d[:, None]
        u = (x - roi[:3]) / (roi[3:] - roi[:3])
        ci = torch.minimum(torch.floor(u * res).long().clamp(min=0), hi_idx)
        occm = binary[ci[..., 0], ci[..., 1], ci[..., 2]] & ((u >= 0) & (u <= 1)).all(-1) & valid
        ri, si = torch.nonzero(occm, as_tuple=True)
        sigma, feat = field.query_density(x[ri, si], return_feat=True)
        alpha = torch.zeros(o.shape[0], S, device=DEV)
        alpha[ri, si] = 1 - torch.exp(-sigma[:, 0] * dt)
        T = torch.cumprod(torch.cat([torch.ones(o.shape[0], 1, device=DEV), 1 - alpha[:, :-1]], 1), 1)
        surv = occm & (T >= eps)
        w = alpha * surv
        w = w * torch.cumprod(torch.cat([torch.ones(o.shape[0], 1, device=DEV), 1 - w[:, :-1]], 1), 1)
        keep = surv[ri, si]
        rgb_s = field.query_rgb(d[ri[keep]], feat[keep])
        ws = w[ri[keep], si[keep]]
        rgb = torch.zeros(o.shape[0], 3, device=DEV).index_add_(0, ri[keep], ws[:, None] * rgb_s)
        op = w.sum(1)
        out_rgb.append(rgb + bkgd * (1 - op[:, None]))
        out_op.append(op)
        out_dep.append((w * tm).sum(1))
        total += int(keep.sum())
    return torch.cat(out_rgb), torch.cat(out_op), torch.cat(out_dep), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-torch", type=int, default=2, help="frames through the torch-composed path (it is slow)")
    args = ap.parse_args()
    field, occ = make_block()
    grid = R.BlockGrid(AABB, occ.binary.to(DEV))
    K, W, H = R.intrinsics("objaverse")
    cams = [look_at((2.7 * math.cos(a) * math.cos(e), 2.7 * math.sin(a) * math.cos(e), 2.7 * math.sin(e)))
            for a, e in [(2 * math.pi * k / 6, el) for el in (0.35, -0.3) for k in range(6)]]
    rays = [R.pixel_rays(c.to(DEV), K, W, H) for c in cams]
    dt, bk = 0.005, torch.ones(3, device=DEV)
    kw = dict(render_step_size=dt, render_bkgd=bk)
    for r in rays[:2]:
        R.render_image(field, grid, r, AABB, **kw)                 # warm-up
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in rays]
    outs, samples = [], 0
    t0 = time.perf_counter()
    for r, (e0, e1) in zip(rays, ev):
        e0.record()
        out = R.render_image(field, grid, r, AABB, **kw)           # (reads the surviving-sample count back: one host sync per frame)
        e1.record()
        outs.append(out)
        samples += out[3]
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    ms_frame = float(np.median(ms))
    # the torch-composed path on the first frames
    nt = max(1, min(args.frames_torch, len(rays)))
    torch_ms, agree, maxd, tsamples = [], [], 0.0, 0
    for r, out in zip(rays[:nt], outs[:nt]):
        torch.cuda.synchronize()
        s = time.perf_counter()
        trgb, top, tdep, tn = torch_composed(field, occ, r, dt, bk)
        torch.cuda.synchronize()
        torch_ms.append(1e3 * (time.perf_counter() - s))
        diff = (trgb - out[0].reshape(-1, 3)).abs().max(dim=1).values
        agree.append(float((diff <= 2e-2).float().mean()))
        maxd = max(maxd, float(diff.max()))
        tsamples += tn
    line = {"bench": "render", "block": "128^3 generated, shell 0.6-1.05", "frames": len(rays), "width": W, "height": H, "render_step_size": dt,
            "ms_per_frame_median": round(ms_frame, 3), "ms_per_frame_min": round(min(ms), 3), "wall_s_all_frames": round(wall, 3),
            "rays_per_s": round(W * H / (ms_frame * 1e-3)), "surviving_samples_per_frame": samples // len(rays),
            "surviving_samples_per_s": round(samples / (sum(ms) * 1e-3)),
            "torch_composed": {"frames": nt, "ms_per_frame": round(float(np.median(torch_ms)), 1), "speedup_fused": round(float(np.median(torch_ms)) / ms_frame, 1),
                               "pixels_within_2e-2_rgb": round(min(agree), 5), "max_abs_rgb_diff": round(maxd, 4),
                               "surviving_samples_fused": sum(o[3] for o in outs[:nt]), "surviving_samples_torch": tsamples}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
