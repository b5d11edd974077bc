"""The dense 1^3 stride-1 trunk convolutions on the implicit GEMM (dreg_conv3d_igemm_ws / _bnstats) and on the streaming kernel
(dreg_conv1_stream / _bnstats, csrc/conv_pointwise.hip), alternated launch group by launch group after warm-up, alone on the chip.
Per shape: microseconds of both (median over the repeats), compulsory bytes (input + output + in-place addend, 2 B per element), TB/s,
the repeat-to-repeat spread (max - min of the repeats' means) and whether the new launch wins by more than the larger spread — the rule
dreg_conv1_stream_use is written from (profiles/pw_stream_by_shape.txt).  Three buffer sets are rotated so that a launch does not find
its operands in the Infinity Cache from the launch before.
usage: python tools/bench_pointwise.py [--repeats 7] [--iters 12]"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreg_nerf_amd import lib as L, ops

args = sys.argv[1:]
REPEATS = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 7
ITERS = int(args[args.index("--iters") + 1]) if "--iters" in args else 12
NBUF = 3
dev = torch.device("cuda", 0)
lib = L.load()
B = 8
# (level, label, Cin, Cout of the product, kind): kind "fwd" = forward with BatchNorm sums, "dgrad" = plain data gradient, "acc" = accumulating data gradient
SHAPES = [
    (32, "fwd 64->256", 64, 256, "fwd"), (32, "fwd 256->64", 256, 64, "fwd"), (32, "dgrad reads 256 writes 64", 256, 64, "dgrad"),
    (32, "dgrad reads 64 adds into 256", 64, 256, "acc"), (32, "fwd 256->128", 256, 128, "fwd"), (32, "dgrad reads 128 adds into 256", 128, 256, "acc"),
    (32, "fwd 64->64", 64, 64, "fwd"), (32, "dgrad 64->64", 64, 64, "dgrad"),
    (16, "fwd 128->512", 128, 512, "fwd"), (16, "dgrad reads 128 adds into 512", 128, 512, "acc"), (16, "dgrad reads 512 writes 128", 512, 128, "dgrad"),
    (16, "fwd 512->128", 512, 128, "fwd"), (16, "fwd 512->256", 512, 256, "fwd"), (16, "dgrad reads 256 writes 512", 256, 512, "dgrad"),
]


def launcher(D, cin, cout, kind, new):
    g = torch.Generator().manual_seed(cin + cout)
    xs = [torch.randn(B, D, D, D, cin, generator=g).to(dev, torch.bfloat16) for _ in range(NBUF)]
    outs = [torch.randn(B, D, D, D, cout, generator=g).to(dev, torch.bfloat16) for _ in range(NBUF)]
    w = (torch.randn(cout, cin, 1, 1, 1, generator=g) / cin ** 0.5).to(dev)
    wpk = ops.packed_weight(w, cin, False, 0)
    V = D ** 3
    sums = torch.empty(B * (V // 128) * cout * 2, dtype=torch.float32, device=dev)
    nws = lib.dreg_conv3d_igemm_workspace_bytes(B, D, D, D, cin, D, D, D, cout, 1, 1, 0, 0, int(kind == "acc"), 0)
    ws = torch.empty(max(int(nws), 16), dtype=torch.uint8, device=dev)
    rpc = ctypes.c_int(0)
    geo = [B, D, D, D, cin, D, D, D, cout, 1, 1, 0]
    st = L.stream()

    def run(i):
        x, o = xs[i % NBUF], outs[i % NBUF]
        if kind == "fwd":
            f = lib.dreg_conv1_stream_bnstats if new else lib.dreg_conv3d_igemm_bnstats
            L.check(f(L.ptr(x), L.ptr(wpk), L.ptr(o), None, None, *geo, 0, 0, 0, 0, 0, L.ptr(ws), int(nws), L.ptr(sums), ctypes.addressof(rpc), st, *((0,) if new else ())), "fwd")
        else:
            add = L.ptr(o) if kind == "acc" else None
            da = [D, D, D, 1] if kind == "acc" else [0, 0, 0, 0]
            f = lib.dreg_conv1_stream if new else lib.dreg_conv3d_igemm_ws
            L.check(f(L.ptr(x), L.ptr(wpk), L.ptr(o), None, add, *geo, 1, 0, *da, 0, 0, L.ptr(ws), int(nws), st, *((0,) if new else ())), kind)
    return run


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(ITERS):
        run(i)
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / ITERS


print(f"# B = {B} grids, bf16; {REPEATS} repeats of {ITERS} launches per arm, alternated; us = median of the repeats' means, spread = max - min of them")
print(f"{'level':>5} {'launch':32} {'MB':>6} | {'igemm us':>9} {'TB/s':>5} {'spread':>6} | {'stream us':>9} {'TB/s':>5} {'spread':>6} | {'gain us':>7} verdict")
for D, label, cin, cout, kind in SHAPES:
    M = B * D ** 3
    nbytes = 2.0 * M * (cin + cout * (2 if kind == "acc" else 1))
    if not lib.dreg_conv1_stream_supported(B, D, D, D, cin, cout, 1, 1, 0, 0, int(kind == "acc"), 1, 0, 0):
        old = launcher(D, cin, cout, kind, False)
        for i in range(6):
            old(i)
        t = sorted(timed(old) for _ in range(REPEATS))
        print(f"{D:>3}^3 {label:32} {nbytes / 1e6:6.0f} | {t[len(t) // 2]:9.1f} {nbytes / t[len(t) // 2] / 1e6:5.2f} {t[-1] - t[0]:6.1f} | {'-':>9} {'-':>5} {'-':>6} | {'-':>7} no instantiation")
        continue
    old, new = launcher(D, cin, cout, kind, False), launcher(D, cin, cout, kind, True)
    for i in range(6):
        old(i); new(i)
    torch.cuda.synchronize()
    to, tn = [], []
    for r in range(REPEATS):
        for arm in ((0, 1) if r % 2 == 0 else (1, 0)):
            (tn if arm else to).append(timed(new if arm else old))
    so, sn = sorted(to), sorted(tn)
    mo, mn = so[len(so) // 2], sn[len(sn) // 2]
    spo, spn = so[-1] - so[0], sn[-1] - sn[0]
    win = mo - mn > max(spo, spn) and sn[-1] < so[0]
    print(f"{D:>3}^3 {label:32} {nbytes / 1e6:6.0f} | {mo:9.1f} {nbytes / mo / 1e6:5.2f} {spo:6.1f} | {mn:9.1f} {nbytes / mn / 1e6:5.2f} {spn:6.1f} | {mo - mn:7.1f} {'stream' if win else 'igemm'}")
    del old, new
    torch.cuda.empty_cache()
