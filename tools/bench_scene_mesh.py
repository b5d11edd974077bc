#!/usr/bin/env python3
"""Surface mesh of a registered SCENE of K = 2, 3, 4 generated 128^3 blocks (tools/bench_render.py make_block, seeds 0..3, under the block poses and
camera centroids of tools/bench_render_scene.py: 20 degrees about z / x / y / (1,1,1), |t| = 0.3, the last block of a scene under no pose) on
scene_lattice(--resolution 256).  Per K:

  fused        ms for SceneField.sample_lattice: ONE launch of scene_density_kernel over the lattice, no position tensor
  composition  ms for the same lattice from the calls the tree had before the fused kernel: node positions in torch, points_to_block, K query_raw,
               the K coverage masks, the K (K - 1) weight terms and the blend as torch elementwise ops (in z-slabs of mesh.QUERY_CHUNK nodes).
               Its result is compared with the fused one (bit for bit where at most one block covers a node, the shared nodes to the weights'
               accuracy).
  count, emit  ms for dreg_mc_count and dreg_mc_emit on the fused lattice; V and F
  skipped      per block, the share of the lattice's 64-node waves in which no lane is covered by it (that block's phase is skipped)

hipEvent pairs after warm-up, median of --rounds, the arms alternated inside a round.  No pass / fail ratio is set.  Writes one JSON object (--out,
default profiles/scene_mesh_bench.json) and prints it.  Needs a GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dreg_nerf_amd import lib as L  # noqa: E402
from dreg_nerf_amd import mesh  # noqa: E402
from dreg_nerf_amd import scene_field as S  # noqa: E402
from bench_pair_mesh import event_ms, skipped_share  # noqa: E402


def composition(sf, origin, spacing, dims, chunk=mesh.QUERY_CHUNK, masks=None):
    """The scene density over the lattice from calls that exist without the fused kernel.  masks (optional list): receives m [n,K] per slab."""
    dev, K = sf.device, sf.K
    nx, ny, nz = dims
    ax = [torch.tensor(origin[c], dtype=torch.float32, device=dev) + torch.arange(dims[c], dtype=torch.float32, device=dev) * torch.tensor(spacing[c], dtype=torch.float32, device=dev)
          for c in range(3)]
    out = torch.empty(nz * ny * nx, dtype=torch.float32, device=dev)
    cen = [torch.tensor(c, device=dev) for c in sf.centers]
    hp = 0.5 * sf.power
    planes = max(1, chunk // (nx * ny))
    for z0 in range(0, nz, planes):
        z1 = min(nz, z0 + planes)
        Z, Y, X = torch.meshgrid(ax[2][z0:z1], ax[1], ax[0], indexing="ij")
        xw = torch.stack([X, Y, Z], dim=-1).reshape(-1, 3)
        xb = [sf.points_to_block(b, xw).contiguous() for b in range(K)]
        m = [sf.covered(b, xb[b]) for b in range(K)]
        sig = [sf.fields[b].query_raw(xb[b])[0] for b in range(K)]
        delta = [((xb[b] - cen[b]) ** 2).sum(dim=1) + 1e-12 for b in range(K)]
        cnt = sum(v.to(torch.int32) for v in m)
        total = None
        for b in range(K):
            s = torch.zeros_like(delta[b])
            lower = torch.zeros_like(m[b])
            d_lo = torch.ones_like(delta[b])
            for o in range(K):
                if o != b:
                    s = s + torch.where(m[o], torch.exp(hp * torch.log(delta[b] / delta[o])), torch.zeros_like(s))
                    if o < b:
                        lower = lower | m[o]
                        d_lo = torch.where(m[o], delta[o], d_lo)
            w = 1.0 / (1.0 + s)
            w = torch.where((cnt == 2) & lower, 1.0 - 1.0 / (1.0 + torch.exp(hp * torch.log(d_lo / delta[b]))), w)      # the pair's omega_hi = 1 - omega_lo
            p = torch.where(m[b], w * sig[b], torch.zeros_like(w))      # (a select, not a product with the mask: an uncovered block's density may be inf)
            total = p if total is None else total + p
        out[z0 * ny * nx:z1 * ny * nx] = total
        if masks is not None:
            masks.append(torch.stack(m, dim=1))
    return out.view(nz, ny, nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--level", type=float, default=mesh.DENSITY_THRE)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_mesh.py measures on the GPU; none found")
    import bench_render
    import bench_render_scene as BRS
    made = [bench_render.make_block(128, seed=s) for s in range(4)]
    poses = [BRS._pose((0, 0, 1), 20.0, (0.2, -0.2, 0.1)), BRS._pose((1, 0, 0), 20.0, (-0.1, 0.2, 0.2)), BRS._pose((0, 1, 0), 20.0, (0.2, 0.1, -0.2)),
             BRS._pose((1, 1, 1), 20.0, (-0.2, -0.1, -0.2))]
    centers = [[0.0, -2.7, 0.5], [2.7, 0.0, 0.5], [0.0, 2.7, 0.5], [-2.7, 0.0, 0.5]]
    dev = torch.device("cuda", 0)
    lib = L.load()
    res = {"blocks": "tools/bench_render.py make_block(128), seeds 0..3; poses and centroids of tools/bench_render_scene.py, the last block of a scene under no pose",
           "resolution": args.resolution, "level": args.level, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "scenes": {},
           "note": "no pass / fail ratio is set; the fused kernel is bound by the hash-grid gathers of the phases that run"}
    for K in (2, 3, 4):
        Pk = poses[:K - 1] + [None]
        sf = S.SceneField([(made[b][0], made[b][1], centers[b], Pk[b]) for b in range(K)])
        origin, spacing, dims = sf.lattice(args.resolution)
        nx, ny, nz = dims
        nodes = nx * ny * nz
        org, spc = (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(*spacing)
        values = sf.sample_lattice(origin, spacing, dims)
        masks = []
        comp = composition(sf, origin, spacing, dims, masks=masks)
        m = torch.cat(masks)
        cnt = m.sum(dim=1).view(nz, ny, nx)
        shared = cnt >= 2
        agree = {"nodes_by_coverage_count": [int((cnt == c).sum()) for c in range(K + 1)],
                 "bit_equal_where_at_most_one_block": bool(torch.equal(values[~shared].view(torch.int32), comp[~shared].view(torch.int32))),
                 "nodes_not_finite": int((~torch.isfinite(values)).sum()), "not_finite_in_the_same_nodes": bool(torch.equal(torch.isfinite(values), torch.isfinite(comp)))}
        fin = shared & torch.isfinite(values) & torch.isfinite(comp)
        agree["max_rel_diff_where_shared"] = float(((values[fin] - comp[fin]).abs() / comp[fin].abs().clamp(min=1e-30)).max()) if int(fin.sum()) else 0.0
        skipped = {f"block_{b}": skipped_share(m[:, b].contiguous(), dims) for b in range(K)}
        skipped["all"] = skipped_share(m.any(dim=1), dims)
        del masks, comp, m, cnt, shared, fin
        nbytes = int(lib.dreg_mc_workspace_bytes(nx, ny, nz))
        ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)

        def count():
            L.check(lib.dreg_mc_count(L.ptr(values), nx, ny, nz, args.level, L.ptr(ws), nbytes, L.ptr(counts), L.stream()), "dreg_mc_count")

        count()
        V, F = counts.tolist()
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)

        def emit():
            L.check(lib.dreg_mc_emit(L.ptr(values), nx, ny, nz, args.level, org, spc, L.ptr(ws), nbytes, L.ptr(verts) if V else None, L.ptr(faces) if F else None,
                                     V, F, L.stream()), "dreg_mc_emit")

        steps = {"fused": lambda: sf.sample_lattice(origin, spacing, dims), "composition": lambda: composition(sf, origin, spacing, dims), "count": count, "emit": emit}
        for _ in range(args.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in steps}
        for _ in range(args.rounds):                         # the arms alternate inside a round: drift of the machine meets all of them alike
            for k, fn in steps.items():
                torch.cuda.synchronize()
                times[k].append(event_ms(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        area, vol = mesh.mesh_area_volume(verts, faces)
        row = {"dims": list(dims), "nodes": nodes, "V": V, "F": F, "area": area, "volume": vol,
               "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
               "composition_over_fused": med["composition"] / med["fused"], "waves_skipped_share": skipped, "fused_vs_composition": agree}
        res["scenes"][f"K{K}"] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
