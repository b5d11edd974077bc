#!/usr/bin/env python3
"""One launch of every branch of the convolution dispatch (igemm_choose / wgrad_choose in csrc/conv.hip) on seeded inputs; prints sha256[:16] of
every output.  The cases are the smallest that reach each branch (the thresholds are in rows, so the volumes stay tiny); the knob-only forms run on
the measurement build through L.probe().  Only the C ABI of include/dreg_nerf.h / dreg_nerf_probe.h is used, so the same file runs against an older
checkout (--tree): run it under `rocprofv3 --kernel-trace` for both and compare (kernel name, grid, workgroup, LDS) row by row and the hashes
(--compare A B reads the two kernel-trace CSVs).  The stamped / "wrong results" measurement forms (wgrad_ring 4..7, wgrad_big 11..13, igemm_probe)
are not run.

usage: python tools/conv_dispatch_sweep.py [--tree CHECKOUT] [--dry]
       python tools/conv_dispatch_sweep.py --compare trace_a.csv trace_b.csv"""
import argparse
import csv
import ctypes
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose dreg_nerf_amd package (and built libraries) to run")
ap.add_argument("--dry", action="store_true", help="no GPU: allocate on the host and check every call's argument list against the binding, launch nothing")
ap.add_argument("--compare", nargs=2, metavar="CSV")
args = ap.parse_args()


def trace_rows(path):
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    dims = sorted(k for k in rows[0] if k.startswith(("Grid_Size", "Workgroup_Size")))      # one column or _X / _Y / _Z, by rocprofv3 version
    return [(r["Kernel_Name"],) + tuple(r[k] for k in dims) + (r["LDS_Block_Size"],) for r in rows]


if args.compare:
    a, b = (trace_rows(p) for p in args.compare)
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    names = sorted({r[0] for r in a if r[0].startswith(("conv_", "void conv_", "wgrad_", "splitk_"))})
    print(f"{len(a)} / {len(b)} kernel launches; first differences: {diff[:5]}")
    print("same sequence of (kernel, grid, workgroup, LDS):", len(a) == len(b) and not diff)
    print("convolution kernels in the trace:", len(names))
    for n in names:
        print("   ", n)
    sys.exit(0 if len(a) == len(b) and not diff else 1)

sys.path.insert(0, args.tree)
import torch
from dreg_nerf_amd import lib as L

DEV = "cpu" if args.dry else "cuda"
BF, F32 = torch.bfloat16, torch.float32
_gen = torch.Generator().manual_seed(1234)


def rnd(*shape, dtype=BF, scale=0.25):
    return (torch.randn(*shape, generator=_gen) * scale).to(dtype).to(DEV)


def call(lib, name, *a):
    """One C-ABI call on the current stream; --dry: only the argument count is checked."""
    sig = dict(L.SIGNATURES, **L.PROBE_SIGNATURES)[name][1]
    assert len(a) + 1 == len(sig), (name, len(a), len(sig))
    if args.dry:
        return
    L.check(getattr(lib, name)(*a, L.stream()), name)


def show(case, **outs):
    if not args.dry:
        torch.cuda.synchronize()
    h = " ".join(f"{k}={hashlib.sha256(v.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]}" for k, v in outs.items())
    print(f"{case:58s} {h}", flush=True)


def odim(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def pack(lib, w, cin_pad, for_dgrad, dt):
    """torch-layout fp32 weight [cout, cin, k, k, k] -> the packed operand of the kernels."""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    if for_dgrad == 2:
        n = (1 if k == 1 else 8) * cin * lib.dreg_conv3d_kpad(1 if k == 1 else 2, cout, dt)
    else:
        n = cout * lib.dreg_conv3d_kpad(k, cin_pad, dt)
    out = torch.zeros(n, dtype=BF if dt == 0 else F32, device=DEV)
    call(lib, "dreg_pack_conv_weight", L.ptr(w), L.ptr(out), cout, cin, cin_pad, k, for_dgrad, dt)
    return out


def igemm(lib, case, B, din, cin, cout, k, s=1, pad=None, *, ws=True, addend=False, dt=0, out_f32=False, relu=0, bias=False, rows=None, api="ws"):
    pad = k // 2 if pad is None else pad
    dout = tuple(odim(d, k, s, pad) for d in din)
    edt = BF if dt == 0 else F32
    odt = F32 if (out_f32 or dt == 1) else BF
    x = rnd(B, *din, cin, dtype=edt)
    wpk = pack(lib, rnd(cout, cin, k, k, k, dtype=F32), cin, 0, dt)
    out = torch.zeros(B, *dout, cout, dtype=odt, device=DEV)
    add = rnd(B, *dout, cout, dtype=odt) if addend else None
    b = rnd(cout, dtype=F32) if bias else None
    geo = (B, *din, cin, *dout, cout, k, s, pad)
    da = dout if addend else (0, 0, 0)
    nws = lib.dreg_conv3d_igemm_workspace_bytes(*geo, 0, int(addend), dt) if ws else 0
    wsp = torch.zeros(max(nws, 4) // 4, dtype=F32, device=DEV) if nws else None
    if rows is not None:
        M = B * dout[0] * dout[1] * dout[2]
        r = torch.randperm(M, generator=_gen)[:rows].sort().values.int().to(DEV)
        call(lib, "dreg_conv3d_igemm_rows", L.ptr(x), L.ptr(wpk), L.ptr(out), L.ptr(b), L.ptr(add), L.ptr(r), rows, *geo, 0, relu, *da, int(addend), int(out_f32))
        show(case, out=out)
    elif api == "ws":
        call(lib, "dreg_conv3d_igemm_ws", L.ptr(x), L.ptr(wpk), L.ptr(out), L.ptr(b), L.ptr(add), *geo, 0, relu, *da, int(addend), dt, int(out_f32 and dt == 0), L.ptr(wsp), nws)
        show(case, out=out)
    elif api == "bnstats":
        V = dout[0] * dout[1] * dout[2]
        part = torch.zeros(B, max(V // 128, 1), cout, 2, dtype=F32, device=DEV)
        rpc = ctypes.c_int(-1)
        call(lib, "dreg_conv3d_igemm_bnstats", L.ptr(x), L.ptr(wpk), L.ptr(out), L.ptr(b), L.ptr(add), *geo, relu, *da, int(addend), L.ptr(wsp), nws, L.ptr(part), ctypes.addressof(rpc))
        show(f"{case} rows_per_chunk={rpc.value}", out=out, sums=part)
    elif api == "defer":
        nsplit, slc = ctypes.c_int(-1), ctypes.c_size_t(0)
        call(lib, "dreg_conv3d_igemm_defer", L.ptr(x), L.ptr(wpk), L.ptr(out), L.ptr(b), L.ptr(add), *geo, 0, relu, *da, int(addend), L.ptr(wsp), nws, None,
             ctypes.addressof(nsplit), ctypes.addressof(slc))
        show(f"{case} nsplit={nsplit.value} slice={slc.value}", out=out, slices=wsp)


def dgrad_s2(lib, case, B, di, cin, cout, k, acc):
    pad = k // 2
    do = odim(di, k, 2, pad)
    g = rnd(B, do, do, do, cout)
    wpk = pack(lib, rnd(cout, cin, k, k, k, dtype=F32), cin, 2, 0)
    din = rnd(B, di, di, di, cin) if acc else torch.zeros(B, di, di, di, cin, dtype=BF, device=DEV)
    call(lib, "dreg_conv3d_dgrad_s2_acc" if acc else "dreg_conv3d_dgrad_s2", L.ptr(g), L.ptr(wpk), L.ptr(din), B, di, di, di, cin, do, do, do, cout, k, pad)
    show(case, din=din)


def wgrad(lib, case, B, dims, cin, cout, k, *, dt=0, use_tr=1, rows=None, occ=False):
    """stride 1, same-size volume"""
    edt = BF if dt == 0 else F32
    D, H, W = dims
    g, x = rnd(B, D, H, W, cout, dtype=edt), rnd(B, D, H, W, cin, dtype=edt)
    dw = torch.zeros(cout, cin, k ** 3, dtype=F32, device=DEV)
    nws = lib.dreg_conv3d_wgrad_workspace_bytes(B, D, H, W, cin, cout, k, dt)
    ws = torch.zeros(nws // 4, dtype=F32, device=DEV)
    geo = (B, D, H, W, cin, cin, D, H, W, cout, k, 1, k // 2)
    if rows is not None:
        r = torch.randperm(B * D * H * W, generator=_gen)[:rows].sort().values.int().to(DEV)
        call(lib, "dreg_conv3d_wgrad_rows", L.ptr(g), L.ptr(x), L.ptr(dw), L.ptr(ws), nws, L.ptr(r), rows, *geo, 0)
    elif occ:
        flags = (torch.rand(B, D, H, generator=_gen) < 0.7).to(torch.uint8).to(DEV)
        call(lib, "dreg_conv3d_wgrad_occ", L.ptr(g), L.ptr(x), L.ptr(dw), L.ptr(ws), nws, *geo, 0, dt, use_tr, L.ptr(flags))
    else:
        call(lib, "dreg_conv3d_wgrad", L.ptr(g), L.ptr(x), L.ptr(dw), L.ptr(ws), nws, *geo, 0, dt, use_tr)
    show(case, dw=dw)


def wgrad_group(lib, case, B, D, cin, cout, k, linear=False):
    """group_fill + group_launch of one layer: the partials the grouped launch leaves in the workspace"""
    g, x = (rnd(B, cout), rnd(B, cin)) if linear else (rnd(B, D, D, D, cout), rnd(B, D, D, D, cin))
    nws = lib.dreg_conv3d_wgrad_workspace_bytes(B, D, D, D, cin, cout, k, 0)
    ws = torch.zeros(nws // 4, dtype=F32, device=DEV)
    nb = lib.dreg_wgrad_group_desc_bytes()
    desc = (ctypes.c_uint8 * nb)()
    var, nblk = ctypes.c_int(0), ctypes.c_int(0)
    if linear:
        rc = lib.dreg_linear_wgrad_group_fill(desc, L.ptr(g), L.ptr(x), L.ptr(ws), nws, B, cin, cout, ctypes.byref(var), ctypes.byref(nblk))
    else:
        rc = lib.dreg_conv3d_wgrad_group_fill(desc, L.ptr(g), L.ptr(x), L.ptr(ws), nws, B, D, D, D, cin, D, D, D, cout, k, 1, k // 2, ctypes.byref(var), ctypes.byref(nblk))
    assert rc == 0, (case, rc)
    d = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).clone().to(DEV)
    call(lib, "dreg_wgrad_group_launch", L.ptr(d), 1, var.value, nblk.value)
    show(f"{case} variant={var.value} nblocks={nblk.value}", partials=ws)


BIG = (64, 32, 32)       # 65,536 rows with Wo % 32 == 0


def run_default(lib):
    igemm(lib, "igemm split-K anti-phase 128x128", 1, (8, 8, 8), 256, 256, 3)
    igemm(lib, "igemm split-K anti-phase 128x64", 1, (8, 8, 8), 256, 64, 3)
    igemm(lib, "igemm split-K four-wave 128x128 bias relu", 32, (8, 8, 8), 256, 256, 3, bias=True, relu=1)
    igemm(lib, "igemm 256x256 anti-phase", 1, BIG, 64, 256, 1)
    igemm(lib, "igemm 1^3 read-modify-write (addend)", 1, BIG, 64, 256, 1, addend=True)
    igemm(lib, "igemm anti-phase 128x128", 1, (16, 16, 16), 128, 128, 3)
    igemm(lib, "igemm anti-phase 128x64 fp32 out", 1, (16, 16, 16), 128, 64, 3, out_f32=True)
    igemm(lib, "igemm four-wave 128x128", 1, (32, 32, 32), 64, 256, 3)
    igemm(lib, "igemm four-wave 128x64", 2, (32, 32, 32), 64, 64, 3)
    igemm(lib, "igemm register-staged stem k5 s2", 1, (16, 16, 16), 8, 64, 5, 2, 2)
    igemm(lib, "igemm register-staged fp32", 1, (8, 8, 8), 64, 64, 3, dt=1)
    igemm(lib, "igemm register-staged stem row list", 1, (16, 16, 16), 8, 64, 5, 2, 2, rows=300)
    igemm(lib, "igemm row list direct-to-LDS", 1, (16, 16, 16), 128, 128, 3, rows=1500)
    for k in (3, 1):
        dgrad_s2(lib, f"dgrad_s2 k{k}", 1, 16, 64, 128, k, False)
        dgrad_s2(lib, f"dgrad_s2_acc k{k}", 1, 16, 64, 128, k, True)
    igemm(lib, "igemm bnstats (emits)", 1, (16, 16, 16), 128, 128, 3, api="bnstats")
    igemm(lib, "igemm bnstats (split-K: does not emit)", 1, (8, 8, 8), 256, 256, 3, api="bnstats")
    igemm(lib, "igemm defer (split-K slices left to the consumer)", 1, (8, 8, 8), 256, 256, 3, api="defer")
    wgrad(lib, "wgrad dense 8-wave fast", 1, BIG, 256, 256, 1)
    wgrad(lib, "wgrad dense 8-wave fast, ragged Kpad 1728", 1, BIG, 64, 256, 3)
    wgrad(lib, "wgrad dense 8-wave general loop (Wo 16)", 1, (64, 64, 16), 64, 256, 3)
    wgrad(lib, "wgrad four-wave 128x128", 8, (16, 16, 16), 256, 256, 1)
    wgrad(lib, "wgrad four-wave 128x64", 4, (16, 16, 16), 256, 256, 1)
    wgrad(lib, "wgrad four-wave 64x128", 4, (16, 16, 16), 64, 64, 3)
    wgrad(lib, "wgrad four-wave 64x64", 1, (4, 4, 4), 64, 64, 1)
    wgrad(lib, "wgrad narrow rule, linear layer 9856 x 256 -> 256", 9856, (1, 1, 1), 256, 256, 1)
    wgrad(lib, "wgrad occupancy flags (Wo 64)", 1, (8, 8, 64), 64, 64, 3, occ=True)
    wgrad(lib, "wgrad row list four-wave", 1, (16, 16, 16), 128, 128, 3, rows=1500)
    wgrad(lib, "wgrad row list 8-wave anti-phase (20,000 rows)", 2, (32, 32, 32), 256, 256, 3, rows=20000)
    wgrad(lib, "wgrad fp32", 1, (8, 8, 8), 64, 64, 3, dt=1, use_tr=0)
    wgrad(lib, "wgrad bf16 use_tr 0", 1, (8, 8, 8), 64, 64, 3, use_tr=0)
    wgrad_group(lib, "wgrad group 128x128", 8, 16, 256, 256, 1)
    wgrad_group(lib, "wgrad group 128x64", 4, 16, 256, 256, 1)
    wgrad_group(lib, "wgrad group 64x128", 4, 16, 64, 64, 3)
    wgrad_group(lib, "wgrad group 64x64", 1, 4, 64, 64, 1)
    wgrad_group(lib, "wgrad group linear 9856 x 256 -> 256", 9856, 1, 256, 256, 1, linear=True)


def run_knobs():
    def with_knob(setter, value, default, fn):
        with L.probe() as p:
            p.set(setter, value, default)
            fn(p.lib, f"[{setter[len('dreg_conv_set_'):]}={value}] ")
    with_knob("dreg_conv_set_glds", 0, 1, lambda lib, t: (igemm(lib, t + "igemm register-staged", 1, (16, 16, 16), 128, 128, 3),
                                                           wgrad(lib, t + "wgrad register-staged bf16", 8, (16, 16, 16), 256, 256, 1)))
    with_knob("dreg_conv_set_glds", 3, 1, lambda lib, t: igemm(lib, t + "igemm 128x256", 1, BIG, 64, 256, 1))
    with_knob("dreg_conv_set_wgrad_big", 1, 3, lambda lib, t: wgrad(lib, t + "wgrad 256x128", 1, BIG, 256, 256, 1))
    for ring in (0, 1, 2, 8):
        with_knob("dreg_conv_set_wgrad_ring", ring, 3, lambda lib, t: wgrad(lib, t + "wgrad dense 8-wave", 1, BIG, 256, 256, 1))
    with L.probe() as p:
        p.set("dreg_conv_set_wgrad_ring", 0, 3)
        p.set("dreg_conv_set_wgrad_pipe", 1, 0)
        wgrad(p.lib, "[wgrad_ring=0 wgrad_pipe=1] wgrad dense 8-wave", 1, BIG, 256, 256, 1)
    with_knob("dreg_conv_set_wgrad_pipe", 1, 0, lambda lib, t: wgrad(lib, t + "wgrad ragged Kpad 1728 (four-wave)", 1, BIG, 64, 256, 3))
    with_knob("dreg_conv_set_wgrad_rows_fast", 0, 1, lambda lib, t: (wgrad(lib, t + "wgrad row list four-wave", 1, (16, 16, 16), 128, 128, 3, rows=1500),
                                                                      wgrad(lib, t + "wgrad row list 20,000 rows", 2, (32, 32, 32), 256, 256, 3, rows=20000)))
    with_knob("dreg_conv_set_row_splits", 0, 1, lambda lib, t: wgrad(lib, t + "wgrad row list 20,000 rows", 2, (32, 32, 32), 256, 256, 3, rows=20000))
    with_knob("dreg_conv_set_narrow_small", 0, 2, lambda lib, t: wgrad(lib, t + "wgrad linear layer 9856 x 256 -> 256", 9856, (1, 1, 1), 256, 256, 1))


run_default(L.load())
run_knobs()
