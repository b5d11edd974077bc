#!/usr/bin/env python3
"""Surface mesh of the generated 128^3 test block (tools/bench_render.py make_block: random hash grid and MLPs) at --resolution 256: a lattice of
257^3 nodes, 68 MB of fp32.

  sampling   ms for the density at every node (dreg_nerf_amd.mesh.sample_density_lattice: query_raw in chunks)
  count      ms for dreg_mc_count (tile pass + the two scan kernels)
  emit       ms for dreg_mc_emit (the 32-byte stamp readback + one launch)
  GB/s       of count and emit against the bytes they must move once: count = the lattice read, one 32-bit word per node written, the (y, z)
             row totals written, read and rewritten by the scan; emit = the lattice and the words read, vertices and faces written.  Halo rows
             that neighbouring workgroups fetch again are NOT counted (they are meant to meet in L2 / Infinity Cache), so the figure is what the
             pass achieves against its minimum traffic.  Beside it the guide's HBM figures: 8.0 TB/s peak, about 6.3 TB/s achieved by a copy.

hipEvent pairs after warm-up, median of --rounds.  Nobody has measured this before: there is no pass / fail ratio.  Writes one JSON object
(--out, default profiles/mesh_bench.json) and prints it.  Needs a GPU."""
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

HBM_PEAK_GBS, HBM_COPY_GBS = 8000.0, 6300.0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--level", type=float, default=mesh.DENSITY_THRE)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU; none found")
    import bench_render
    field, _occ = bench_render.make_block(128)
    dev = torch.device("cuda", 0)
    lib = L.load()
    n = args.resolution + 1
    origin, spacing = mesh.lattice_of(field._aabb_host(), args.resolution)
    org, spc = (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(*spacing)
    values = mesh.sample_density_lattice(field, args.resolution)
    nbytes = int(lib.dreg_mc_workspace_bytes(n, n, n))
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)

    def count():
        L.check(lib.dreg_mc_count(L.ptr(values), n, n, n, args.level, L.ptr(ws), nbytes, L.ptr(counts), L.stream()), "dreg_mc_count")

    count()
    V, F = counts.tolist()
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)

    def emit():
        L.check(lib.dreg_mc_emit(L.ptr(values), n, n, n, args.level, org, spc, L.ptr(ws), nbytes, L.ptr(verts), L.ptr(faces), V, F, L.stream()), "dreg_mc_emit")

    steps = {"sampling": lambda: mesh.sample_density_lattice(field, args.resolution), "count": count, "emit": emit}
    for _ in range(args.warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, fn in steps.items():
            torch.cuda.synchronize()
            times[k].append(event_ms(fn))
    nodes, rows = n ** 3, n * n
    moved = {"count": 4 * nodes + 4 * nodes + 8 * rows + 16 * rows, "emit": 4 * nodes + 4 * nodes + 8 * rows + 12 * V + 12 * F}
    med = {k: statistics.median(v) for k, v in times.items()}
    area, vol = mesh.mesh_area_volume(verts, faces)
    res = {"block": "tools/bench_render.py make_block(128), seed 0", "resolution": args.resolution, "nodes": nodes, "level": args.level, "V": V, "F": F,
           "area": area, "volume": vol, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
           "bytes_moved": moved, "gb_per_s": {k: moved[k] / (med[k] * 1e-3) / 1e9 for k in moved},
           "workspace_bytes": nbytes, "hbm_gb_per_s_guide": {"peak": HBM_PEAK_GBS, "copy_measured": HBM_COPY_GBS},
           "note": "bytes_moved is the minimum traffic of each pass (halo re-reads excluded); no pass / fail ratio is set"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
