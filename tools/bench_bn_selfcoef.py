"""The large-path training BatchNorm with and without its finalize launch, shape by shape (every train-mode large-path shape of the step, B = 8).

forward:  bn_finalize_kernel + bn_apply_cols_kernel (dreg_bn3d_fwd_from_sums)      against  bn_apply_self_kernel (dreg_bn3d_fwd_self_coef)
backward: bn_partial_kernel<., 1> + bn_bwd_finalize_kernel + bn_bwd_apply_cols_kernel (dreg_bn3d_bwd)
                                                                                    against  bn_partial_kernel<., 1> + bn_bwd_apply_self_kernel
Both arms start from the same chunk sums; the fused arm leaves the cross-grid tail to the pass's batched launch (one launch for all layers, not
timed here).  The arms alternate, HIP events around `--n` launches, `--reps` repeats, three rotated buffer sets so that a launch does not find its
operands in the caches its own previous launch left.  Prints the median and the repeat-to-repeat range of each arm and the verdict
dreg_bn_self_coef_use is written from (fused faster by more than the larger of the two ranges).
usage: python tools/bench_bn_selfcoef.py [--wgs 512,1024,2048] [--n 20] [--reps 7]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreg_nerf_amd import lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--wgs", default="512")
ap.add_argument("--n", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = L.use_probe()
B, SETS = 8, 3
#        V3, C, res, res_ss
SHAPES = ((32, 64, 0, 0), (32, 128, 0, 0), (32, 256, 0, 0), (32, 256, 1, 0), (32, 256, 1, 1), (16, 128, 0, 0), (16, 256, 0, 0), (16, 512, 0, 0), (16, 512, 1, 0))


def timed(fns, n):
    """us per call of each fn, the fns taken in turn"""
    out = []
    for fn in fns:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i % SETS)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    return out


def report(tag, chain, fused):
    mc, mf = statistics.median(chain), statistics.median(fused)
    rc, rf = max(chain) - min(chain), max(fused) - min(fused)
    verdict = "fused" if mc - mf > max(rc, rf) else ("chain" if mf - mc > max(rc, rf) else "tie")
    print(f"  {tag}: chain {mc:7.1f} us (range {rc:4.1f})  fused {mf:7.1f} us (range {rf:4.1f})  diff {mc - mf:+6.1f} us  -> {verdict}", flush=True)


for wgs in [int(w) for w in args.wgs.split(",")]:
    lib.dreg_bn_set_self_wgs(wgs)
    print(f"workgroup bound {wgs}")
    for V3, C, with_res, with_rss in SHAPES:
        V = V3 ** 3
        n = B * V * C
        nch = lib.dreg_bn_num_chunks(V)
        rpc = V // nch
        frpc = min(rpc, 128)          # forward: the chunk sums come from the convolution epilogues, 128 rows per chunk (their values do not matter here)
        S = []
        for _ in range(SETS):
            d = dict(x=torch.randn(n, device=dev).bfloat16(), dy=torch.randn(n, device=dev).bfloat16(), y=torch.empty(n, device=dev, dtype=torch.bfloat16),
                     dx=torch.empty(n, device=dev, dtype=torch.bfloat16), res=torch.randn(n, device=dev).bfloat16() if with_res else None,
                     dres=torch.empty(n, device=dev, dtype=torch.bfloat16) if with_res else None, sums=torch.zeros(B * (V // min(V // nch, 128)) * C * 2, device=dev),
                     ws=torch.zeros(B * nch * C * 2, device=dev), ss=torch.zeros(B * C * 2, device=dev), mr=torch.zeros(B * C * 2, device=dev),
                     coef=torch.zeros(B * C * 2, device=dev), keep=torch.zeros(B * C * 2, device=dev, dtype=torch.float64),
                     rss=torch.ones(B * C * 2, device=dev) if with_rss else None)
            S.append(d)
        g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        for d in S:   # the saved tensors the backward reads
            L.check(lib.dreg_bn3d_fwd(L.ptr(d["x"]), None, L.ptr(d["y"]), L.ptr(g), L.ptr(b), L.ptr(rm), L.ptr(rv), L.ptr(d["ss"]), L.ptr(d["mr"]), L.ptr(d["ws"]),
                                      B, V, C, 1e-5, 0.1, 1, 1, 0, L.stream()), "sums")
        ex = None
        if with_rss:
            import ctypes

            class BnExtra(ctypes.Structure):
                _fields_ = [("res_scale_shift", ctypes.c_void_p), ("splitk_part", ctypes.c_void_p), ("splitk_nsplit", ctypes.c_int), ("splitk_slice", ctypes.c_size_t)]
            ex = [BnExtra(L.ptr(d["rss"]), None, 0, 0) for d in S]

        def f_chain(i):
            d = S[i]
            if with_rss:
                L.check(lib.dreg_bn3d_fwd_ex(L.ptr(d["x"]), L.ptr(d["res"]), L.ptr(d["y"]), L.ptr(g), L.ptr(b), L.ptr(rm), L.ptr(rv), L.ptr(d["ss"]), L.ptr(d["mr"]),
                                             L.ptr(d["sums"]), B, V, C, 1e-5, 0.1, 1, 1, 0, None, None, frpc, ctypes.addressof(ex[i]), L.stream()), "fwd chain")
            else:
                L.check(lib.dreg_bn3d_fwd_from_sums(L.ptr(d["x"]), L.ptr(d["res"]), L.ptr(d["y"]), L.ptr(g), L.ptr(b), L.ptr(rm), L.ptr(rv), L.ptr(d["ss"]), L.ptr(d["mr"]),
                                                    L.ptr(d["sums"]), frpc, B, V, C, 1e-5, 0.1, 1, 0, L.stream()), "fwd chain")

        def f_fused(i):
            d = S[i]
            L.check(lib.dreg_bn3d_fwd_self_coef(L.ptr(d["x"]), L.ptr(d["res"]), L.ptr(d["y"]), L.ptr(g), L.ptr(b), L.ptr(d["ss"]), L.ptr(d["mr"]), L.ptr(d["sums"]), frpc,
                                                B, V, C, 1e-5, 1, 0, L.ptr(d["keep"]), L.ptr(d["rss"]), L.stream()), "fwd fused")

        def b_chain(i):
            d = S[i]
            L.check(lib.dreg_bn3d_bwd(L.ptr(d["x"]), L.ptr(d["dy"]), L.ptr(d["y"]) if with_res else None, L.ptr(d["ss"]), L.ptr(d["mr"]), L.ptr(d["dx"]), L.ptr(d["dres"]),
                                      L.ptr(dg), L.ptr(db), L.ptr(d["coef"]), L.ptr(d["ws"]), B, V, C, 1, 1, 0, L.stream()), "bwd chain")

        def b_fused(i):
            d = S[i]
            L.check(lib.dreg_bn3d_bwd_self_coef(L.ptr(d["x"]), L.ptr(d["dy"]), L.ptr(d["y"]) if with_res else None, L.ptr(d["ss"]), L.ptr(d["mr"]), L.ptr(d["dx"]),
                                                L.ptr(d["dres"]), L.ptr(d["ws"]), B, V, C, 1, 0, L.ptr(d["keep"]), L.stream()), "bwd fused")

        timed((f_chain, f_fused, b_chain, b_fused), 3)       # warm-up
        T = [timed((f_chain, f_fused, b_chain, b_fused), args.n) for _ in range(args.reps)]
        fc, ff, bc, bf = zip(*T)
        rows = lib.dreg_bn_self_coef_rows(B, V, C, 0)
        print(f"{V3}^3 x {C:4d}{' +res' if with_res else '     '}{'_ss' if with_rss else '   '} chunks fwd/bwd {V // frpc:3d}/{nch:3d} rows/workgroup {rows:4d} "
              f"use fwd/bwd {lib.dreg_bn_self_coef_use(B, V, C, 0, 0)}/{lib.dreg_bn_self_coef_use(B, V, C, 0, 1)}")
        report("forward ", fc, ff)
        report("backward", bc, bf)
        del S
        torch.cuda.empty_cache()
