"""Each row-local chain of an encoder layer as ONE row-panel launch (dreg_ps_panel_fwd / dreg_ps_panel_bwd) against the launches it
replaces (linear -> LayerNorm -> linear; data gradient -> LayerNorm backward -> data gradient), at the benchmark's row count.  HIP events around 20 back-to-back launches on one stream, after a warm-up.
usage: python tools/bench_ps_panel.py [--rows 9752] [--reps 20] [--json out.json]"""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreg_nerf_amd import lib as L

args = sys.argv[1:]
opt = lambda k, d: type(d)(args[args.index(k) + 1]) if k in args else d
R, REPS, OUT = opt("--rows", 9752), opt("--reps", 20), opt("--json", "")
CHAINS = [("F1 out_proj_self(+x) -> LN2(+pe) -> in_proj_cross", 256, 768, 0, True),
          ("F2 out_proj_cross(+xa) -> LN3 -> linear1+ReLU", 256, 1024, 1, False),
          ("F3 linear2(+xb) -> LN1(+pe) -> in_proj_self", 1024, 768, 0, True)]
lib = L.load()
dev = torch.device("cuda", 0)
S = L.stream


def pack(w):
    out = torch.empty(w.shape[0], lib.dreg_conv3d_kpad(1, w.shape[1], L.DT_BF16), dtype=torch.bfloat16, device=dev)
    L.check(lib.dreg_pack_conv_weight(L.ptr(w), L.ptr(out), w.shape[0], w.shape[1], w.shape[1], 1, 0, L.DT_BF16, S()), "pack")
    return out


def linear(x, wpk, bias, res, out, cin, cout, relu, f32):
    a = 1 if res is not None else 0
    L.check(lib.dreg_conv3d_igemm_ws(L.ptr(x), L.ptr(wpk), L.ptr(out), L.ptr(bias), L.ptr(res), R, 1, 1, 1, cin, 1, 1, 1, cout, 1, 1, 0, 0, relu,
                                     a, a, a, a, 0, f32, None, 0, S()), "igemm")


def timed(fn):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / REPS


rows = []
for name, K1, N2, relu, with_pe in CHAINS:
    a1 = torch.randn(R, K1, device=dev).to(torch.bfloat16)
    p1, p2 = pack(torch.randn(256, K1, device=dev) * K1 ** -0.5), pack(torch.randn(N2, 256, device=dev) / 16)
    b1, b2, gm, bt = torch.randn(256, device=dev), torch.randn(N2, device=dev), torch.ones(256, device=dev), torch.zeros(256, device=dev)
    res, pe = torch.randn(R, 256, device=dev), (torch.randn(R, 256, device=dev) if with_pe else None)
    x, h, st, o = (torch.empty(R, 256, device=dev), torch.empty(R, 256, device=dev, dtype=torch.bfloat16), torch.empty(R, 2, device=dev),
                   torch.empty(R, N2, device=dev, dtype=torch.bfloat16))
    g1 = lambda: linear(a1, p1, b1, res, x, K1, 256, 0, 1)
    ln = lambda: L.check(lib.dreg_layernorm_fwd(L.ptr(x), L.ptr(gm), L.ptr(bt), L.ptr(pe), L.ptr(h), L.ptr(st), R, 256, 1e-5, 0, S()), "ln")
    g2 = lambda: linear(h, p2, b2, None, o, 256, N2, relu, 0)
    pn = lambda: L.check(lib.dreg_ps_panel_fwd(L.ptr(a1), L.ptr(p1), L.ptr(b1), L.ptr(res), L.ptr(x), L.ptr(gm), L.ptr(bt), L.ptr(pe), L.ptr(h), L.ptr(st),
                                               L.ptr(p2), L.ptr(b2), L.ptr(o), R, K1, N2, relu, 1e-5, S()), "panel")
    chain = lambda: (g1(), ln(), g2())
    parts = [timed(g1), timed(ln), timed(g2)]
    r = {"chain": name, "rows": R, "K1": K1, "N2": N2, "launch_us": [round(v, 2) for v in parts], "launch_sum_us": round(sum(parts), 2),
         "chain_us": round(timed(chain), 2), "panel_us": round(timed(pn), 2)}
    rows.append(r)
    print(f"{name}: launches {' + '.join(f'{v:.1f}' for v in parts)} = {sum(parts):.1f} us (back to back {r['chain_us']:.1f} us), panel {r['panel_us']:.1f} us", flush=True)


def pack_t(w):
    out = torch.empty(w.shape[1], lib.dreg_conv3d_kpad(1, w.shape[0], L.DT_BF16), dtype=torch.bfloat16, device=dev)
    L.check(lib.dreg_pack_conv_weight(L.ptr(w), L.ptr(out), w.shape[0], w.shape[1], w.shape[1], 1, 1, L.DT_BF16, S()), "pack")
    return out


def dgrad(g, wpk_t, gx, cin, cout):
    L.check(lib.dreg_conv3d_igemm_ws(L.ptr(g), L.ptr(wpk_t), L.ptr(gx), None, None, R, 1, 1, 1, cout, 1, 1, 1, cin, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, None, 0, S()), "igemm")


for name, K1, N2, inpl in [("B1 dgrad linear1 -> LN3' (+G) -> dgrad out_proj_cross", 1024, 256, False),
                           ("B2 dgrad in_proj_cross -> LN2' (+Gb) -> dgrad out_proj_self", 768, 256, False),
                           ("B3 dgrad in_proj_self -> LN1' (+Ga +Gprev)", 768, 0, True)]:
    g1 = torch.randn(R, K1, device=dev).to(torch.bfloat16)
    p1, p2 = pack_t(torch.randn(K1, 256, device=dev) * K1 ** -0.5), pack_t(torch.randn(256, 256, device=dev) / 16)
    x, add, gm = torch.randn(R, 256, device=dev), torch.randn(R, 256, device=dev), torch.ones(256, device=dev)
    st = torch.cat([x.mean(1, keepdim=True), 1.0 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)], 1).contiguous()
    dH, dx, bf, o = (torch.empty(R, 256, device=dev, dtype=torch.bfloat16), torch.zeros(R, 256, device=dev), torch.empty(R, 256, device=dev, dtype=torch.bfloat16),
                     torch.empty(R, 256, device=dev, dtype=torch.bfloat16))
    part = torch.empty(lib.dreg_layernorm_bwd_workspace_bytes(R) // 4, device=dev)
    add2 = dx if inpl else None
    g1f = lambda: dgrad(g1, p1, dH, 256, K1)
    ln = lambda: L.check(lib.dreg_layernorm_bwd_parts(L.ptr(x), L.ptr(dH), None, L.ptr(gm), L.ptr(st), L.ptr(dx), L.ptr(add), L.ptr(add2), L.ptr(bf), L.ptr(part),
                                                      R, 256, 0, S()), "ln")
    g2f = (lambda: dgrad(bf, p2, o, 256, 256)) if N2 else (lambda: None)
    pn = lambda: L.check(lib.dreg_ps_panel_bwd(L.ptr(g1), L.ptr(p1), L.ptr(x), L.ptr(st), L.ptr(gm), L.ptr(add), L.ptr(add2), L.ptr(dx), L.ptr(bf), L.ptr(part),
                                               L.ptr(p2) if N2 else None, L.ptr(o) if N2 else None, R, K1, N2, S()), "panel")
    chain = lambda: (g1f(), ln(), g2f())
    parts = [timed(g1f), timed(ln)] + ([timed(g2f)] if N2 else [])
    r = {"chain": name, "rows": R, "K1": K1, "N2": N2, "launch_us": [round(v, 2) for v in parts], "launch_sum_us": round(sum(parts), 2),
         "chain_us": round(timed(chain), 2), "panel_us": round(timed(pn), 2)}
    rows.append(r)
    print(f"{name}: launches {' + '.join(f'{v:.1f}' for v in parts)} = {sum(parts):.1f} us (back to back {r['chain_us']:.1f} us), panel {r['panel_us']:.1f} us", flush=True)
if OUT:
    json.dump(rows, open(OUT, "w"), indent=1)
