#!/usr/bin/env python3
"""Surface mesh of a registered PAIR of generated 128^3 blocks (tools/bench_render.py make_block, seeds 3 and 5, under the pose of
tests/test_hip_pair_field.py: 25 degrees about z, t = (-0.13, 0.02, 0.02)) on pair_lattice(--resolution 256).

  fused        ms for PairField.sample_lattice: ONE launch of the density-field kernel (dreg_pair_density) over the lattice, no position tensor
  composition  ms for the same lattice from the calls the tree had before the fused kernel: node positions in torch, the source-frame positions,
               two query_raw, the two coverage masks, the weight and the blend as torch elementwise ops (in z-slabs of mesh.QUERY_CHUNK nodes, as
               mesh.sample_density_lattice walks a block's lattice).  The baseline the fused kernel is judged against; its result is compared
               with the fused one (sigma bit for bit where one block alone covers a node, the shared nodes to the weight's accuracy).
  count, emit  ms for dreg_mc_count and dreg_mc_emit on the fused lattice; V and F
  skipped      the share of the lattice's 64-node waves in which no lane is covered by the source / by the target (that block's phase is skipped)
  GB/s         of the fused launch against the lattice's minimum traffic: one fp32 written per node (positions are formed in the lanes)

hipEvent pairs after warm-up, median of --rounds.  No pass / fail ratio is set.  Writes one JSON object (--out, default
profiles/pair_mesh_bench.json) and prints it.  Needs a GPU."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dreg_nerf_amd import lib as L  # noqa: E402
from dreg_nerf_amd import mesh  # noqa: E402
from dreg_nerf_amd import pair_field as P  # noqa: E402

C_SRC, C_TGT = [0.3, -2.2, 0.6], [2.1, 0.4, 0.5]


def pose():
    a = math.radians(25.0)
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    M[:3, 3] = torch.tensor([-0.13, 0.02, 0.02], dtype=torch.float64)
    return M


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def composition(pf, origin, spacing, dims, chunk=mesh.QUERY_CHUNK, masks=None):
    """The pair density over the lattice from calls that exist without the fused kernel.  masks (optional list): receives (m_src, m_tgt) per slab."""
    dev = pf.device
    nx, ny, nz = dims
    ax = [torch.tensor(origin[c], dtype=torch.float32, device=dev) + torch.arange(dims[c], dtype=torch.float32, device=dev) * torch.tensor(spacing[c], dtype=torch.float32, device=dev)
          for c in range(3)]
    out = torch.empty(nz * ny * nx, dtype=torch.float32, device=dev)
    c_s, c_t = torch.tensor(C_SRC, device=dev), torch.tensor(C_TGT, device=dev)
    planes = max(1, chunk // (nx * ny))
    for z0 in range(0, nz, planes):
        z1 = min(nz, z0 + planes)
        Z, Y, X = torch.meshgrid(ax[2][z0:z1], ax[1], ax[0], indexing="ij")
        xt = torch.stack([X, Y, Z], dim=-1).reshape(-1, 3)
        xs = pf.points_to_source(xt).contiguous()
        m_s, m_t = pf.covered(0, xs), pf.covered(1, xt)
        s_s, s_t = pf.src.query_raw(xs)[0], pf.tgt.query_raw(xt)[0]
        q = (((xs - c_s) ** 2).sum(dim=1) + 1e-12) / (((xt - c_t) ** 2).sum(dim=1) + 1e-12)
        w = 1.0 / (1.0 + torch.exp(0.5 * pf.power * torch.log(q)))
        one, zero = torch.ones_like(w), torch.zeros_like(w)
        w_s = torch.where(m_s, torch.where(m_t, w, one), zero)
        w_t = torch.where(m_t, torch.where(m_s, 1.0 - w, one), zero)
        out[z0 * ny * nx:z1 * ny * nx] = w_s * (s_s * m_s) + w_t * (s_t * m_t)
        if masks is not None:
            masks.append((m_s, m_t))
    return out.view(nz, ny, nx)


def skipped_share(mask, dims):
    """Share of the lattice's waves (64 x-contiguous nodes of one (y,z) row) in which no lane has the mask set."""
    nx, ny, nz = dims
    pad = (nx + 63) // 64 * 64
    m = torch.zeros(nz * ny, pad, dtype=torch.bool, device=mask.device)
    m[:, :nx] = mask.view(nz * ny, nx)
    return 1.0 - float(m.view(nz * ny, pad // 64, 64).any(dim=2).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--level", type=float, default=mesh.DENSITY_THRE)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_mesh.py measures on the GPU; none found")
    import bench_render
    (sf, so), (tf, to) = bench_render.make_block(128, seed=3), bench_render.make_block(128, seed=5)
    dev = torch.device("cuda", 0)
    pf = P.PairField(sf, so, tf, to, pose(), C_SRC, C_TGT)
    lib = L.load()
    origin, spacing, dims = pf.lattice(args.resolution)
    nx, ny, nz = dims
    nodes = nx * ny * nz
    org, spc = (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(*spacing)
    values = pf.sample_lattice(origin, spacing, dims)
    masks = []
    comp = composition(pf, origin, spacing, dims, masks=masks)
    m_s, m_t = torch.cat([m[0] for m in masks]), torch.cat([m[1] for m in masks])
    single = (m_s ^ m_t).view(nz, ny, nx)
    both = (m_s & m_t).view(nz, ny, nx)
    agree = {"nodes_one_block": int(single.sum()), "nodes_both_blocks": int(both.sum()), "nodes_no_block": int((~(m_s | m_t)).sum()),
             "bit_equal_where_one_or_no_block": bool(torch.equal(values[~both].view(torch.int32), comp[~both].view(torch.int32))),
             "max_rel_diff_where_both": float(((values[both] - comp[both]).abs() / comp[both].abs().clamp(min=1e-30)).max()) if int(both.sum()) else 0.0}
    skipped = {"source": skipped_share(m_s, dims), "target": skipped_share(m_t, dims), "both": skipped_share(m_s | m_t, dims)}
    del masks, comp, m_s, m_t, single, both
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

    steps = {"fused": lambda: pf.sample_lattice(origin, spacing, dims), "composition": lambda: composition(pf, origin, spacing, dims), "count": count, "emit": emit}
    for _ in range(args.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(args.rounds):                         # the steps alternate inside a round: drift of the machine meets all of them alike
        for k, fn in steps.items():
            torch.cuda.synchronize()
            times[k].append(event_ms(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    area, vol = mesh.mesh_area_volume(verts, faces)
    res = {"blocks": "tools/bench_render.py make_block(128), seeds 3 (source) and 5 (target), pose 25 deg about z, t = (-0.13, 0.02, 0.02)",
           "resolution": args.resolution, "dims": list(dims), "nodes": nodes, "level": args.level, "V": V, "F": F, "area": area, "volume": vol,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
           "composition_over_fused": med["composition"] / med["fused"],
           "waves_skipped_share": skipped, "fused_vs_composition": agree,
           "min_bytes_fused": 4 * nodes, "gb_per_s_fused": 4 * nodes / (med["fused"] * 1e-3) / 1e9,
           "note": "min_bytes_fused is one fp32 written per node; the kernel is bound by the hash-grid gathers, not by that traffic; no pass / fail ratio is set"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
