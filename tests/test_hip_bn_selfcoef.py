"""GPU: the self-coefficient BatchNorm apply passes (bn_apply_self_kernel / bn_bwd_apply_self_kernel of csrc/fpn_ops.hip: no finalize launch)
against the three-launch form, bit for bit.

Both arms read the SAME chunk sums (forward: left by a bn_partial_kernel<., 0> launch, the layout the convolution epilogues write; backward: each
arm's own bn_partial_kernel<., 1> launch over the same operands), so every output must be torch.equal: y, scale_shift, mean_rstd, dx, dres and —
after the batched tail over the fp64 keep pairs — running_mean, running_var, dgamma, dbeta (accumulate 0 and 1).  Outputs are NaN beforehand.
The shapes are the smallest that reach each path: chunk counts around the 64-lane stride of the sums (1, 2, 63, 64, 65, 130), grid counts
1 / 3 / 8 / 9, channel widths below, at and above the 128-channel bound of one workgroup (ragged last slab included), and a volume whose row
count is not a multiple of the apply pass's rows per workgroup."""
import ctypes

import numpy as np
import pytest
import torch

import bn_cases as N
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF, F32 = torch.bfloat16, torch.float32
TAIL_DT = np.dtype([("a", "<u8"), ("b", "<u8"), ("o0", "<u8"), ("o1", "<u8"), ("B", "<i4"), ("V", "<i4"), ("C", "<i4"), ("block0", "<i4")])
EPS, MOM = 1e-5, 0.1

# (B, V, C, dtype)        chunks (dreg_bn_num_chunks)
CHUNK_CASES = [
    (1, 8, 8, 0),         # 1
    (3, 16, 8, 1),        # 2
    (8, 504, 8, 0),       # 63
    (9, 2048, 8, 0),      # 64
    (3, 2080, 8, 1),      # 65
    (1, 16640, 8, 0),     # 130
]
CHUNKS = [1, 2, 63, 64, 65, 130]
WIDTH_CASES = [
    (3, 1024, 64, 0),
    (8, 1024, 128, 0),
    (3, 1024, 136, 0),    # 128 + one granule: ragged second slab
    (9, 1248, 264, 0),    # three slabs, 39 chunks x 9 x 3 workgroups > 512: rows per workgroup double twice to 128, 1248 = 9.75 x 128
    (3, 1024, 136, 1),    # fp32: 34 granules of 4 channels, slabs of 32
    (1, 1024, 264, 1),
]
FWD_VARIANTS = ["plain", "relu", "res", "res_ss"]
BWD_VARIANTS = ["remask", "relu_y", "dres_gstored", "norelu"]


def nanf(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def call(lib, name, *a):
    L.check(getattr(lib, name)(*a, L.stream()), name)


def tail_table(b, o0, o1, B, V, C):
    t = np.zeros(1, TAIL_DT)
    t[0] = (0, b.data_ptr(), o0.data_ptr(), o1.data_ptr(), B, V, C, 0)        # a = NULL: b = fp64 pairs
    return torch.from_numpy(t.view(np.uint8)).to(DEV), (C + 255) // 256


def operands(B, V, C, dt, seed):
    g = torch.Generator().manual_seed(seed)
    T = BF if dt == 0 else F32
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(T=T, x=(r(B, V, C) * 1.5 + r(1, 1, C)).to(DEV, T), res=r(B, V, C).to(DEV, T), dy=r(B, V, C).to(DEV, T),
                gamma=(1 + 0.3 * r(C)).to(DEV), beta=(0.2 * r(C)).to(DEV), rm=r(C).to(DEV), rv=(1 + r(C).abs()).to(DEV),
                res_ss=torch.stack([1 + 0.2 * r(B, C), 0.1 * r(B, C)], -1).contiguous().to(DEV), dg0=r(C).to(DEV), db0=r(C).to(DEV))


def run_forward(lib, B, V, C, dt, variant, o):
    relu = int(variant != "plain")
    res = o["res"] if variant in ("res", "res_ss") else None
    ex = N.BnExtra(L.ptr(o["res_ss"]) if variant == "res_ss" else None, None, 0, 0)
    nch = lib.dreg_bn_num_chunks(V)
    assert V % nch == 0
    rpc = V // nch
    # the chunk sums, as a statistics pass leaves them
    ws = nanf(B * nch * C * 2)
    junk = [nanf(B, V, C, dtype=o["T"]), o["rm"].clone(), o["rv"].clone(), nanf(B, C, 2), nanf(B, C, 2)]
    call(lib, "dreg_bn3d_fwd", L.ptr(o["x"]), None, L.ptr(junk[0]), L.ptr(o["gamma"]), L.ptr(o["beta"]), L.ptr(junk[1]), L.ptr(junk[2]), L.ptr(junk[3]),
         L.ptr(junk[4]), L.ptr(ws), B, V, C, EPS, MOM, 1, 0, dt)
    assert torch.isfinite(ws).all()
    sums0 = ws.clone()
    # three launches from the sums
    a = dict(y=nanf(B, V, C, dtype=o["T"]), ss=nanf(B, C, 2), mr=nanf(B, C, 2), rm=o["rm"].clone(), rv=o["rv"].clone())
    call(lib, "dreg_bn3d_fwd_ex", L.ptr(o["x"]), L.ptr(res), L.ptr(a["y"]), L.ptr(o["gamma"]), L.ptr(o["beta"]), L.ptr(a["rm"]), L.ptr(a["rv"]), L.ptr(a["ss"]),
         L.ptr(a["mr"]), L.ptr(ws), B, V, C, EPS, MOM, 1, relu, dt, None, None, rpc, ctypes.addressof(ex))
    # one launch + the batched tail
    b = dict(y=nanf(B, V, C, dtype=o["T"]), ss=nanf(B, C, 2), mr=nanf(B, C, 2), rm=o["rm"].clone(), rv=o["rv"].clone())
    keep = nanf(B, C, 2, dtype=torch.float64)
    assert lib.dreg_bn_self_coef_supported(B, V, C, dt) == 1
    call(lib, "dreg_bn3d_fwd_self_coef", L.ptr(o["x"]), L.ptr(res), L.ptr(b["y"]), L.ptr(o["gamma"]), L.ptr(o["beta"]), L.ptr(b["ss"]), L.ptr(b["mr"]), L.ptr(ws),
         rpc, B, V, C, EPS, relu, dt, L.ptr(keep), L.ptr(o["res_ss"]) if variant == "res_ss" else None)
    assert torch.equal(b["rm"], o["rm"]) and torch.equal(b["rv"], o["rv"])
    td, blocks = tail_table(keep, b["rm"], b["rv"], B, V, C)
    call(lib, "dreg_bn_running_update_batched", L.ptr(td), 1, 0, blocks, MOM)
    torch.cuda.synchronize()
    assert torch.equal(ws, sums0)
    assert torch.isfinite(a["y"].float()).all() and torch.isfinite(a["rv"]).all()
    for k in a:
        assert torch.equal(a[k], b[k]), f"forward {variant}: {k} differs ({int((a[k] != b[k]).sum())} of {a[k].numel()})"
    assert torch.equal(keep[..., 0].float(), a["mr"][..., 0])
    return a


def run_backward(lib, B, V, C, dt, variant, o, fw):
    relu = int(variant != "norelu")
    y = None if variant in ("remask", "norelu") else fw["y"]
    with_dres = variant == "dres_gstored"
    nch = lib.dreg_bn_num_chunks(V)
    outs = []
    for arm in (0, 1):
        dx = nanf(B, V, C, dtype=o["T"])
        dres = nanf(B, V, C, dtype=o["T"]) if with_dres else None
        ws = nanf(B * nch * C * 2)
        r = dict(dx=dx)
        if with_dres:
            r["dres"] = dres
        if arm == 0:
            for acc in (0, 1):
                dg, db = (o["dg0"].clone(), o["db0"].clone()) if acc else (nanf(C), nanf(C))
                call(lib, "dreg_bn3d_bwd", L.ptr(o["x"]), L.ptr(o["dy"]), L.ptr(y), L.ptr(fw["ss"]), L.ptr(fw["mr"]), L.ptr(dx), L.ptr(dres), L.ptr(dg), L.ptr(db),
                     L.ptr(nanf(B, C, 2)), L.ptr(ws), B, V, C, relu, acc, dt)
                r[f"dgamma{acc}"], r[f"dbeta{acc}"] = dg, db
        else:
            keep = nanf(B, C, 2, dtype=torch.float64)
            call(lib, "dreg_bn3d_bwd_self_coef", L.ptr(o["x"]), L.ptr(o["dy"]), L.ptr(y), L.ptr(fw["ss"]), L.ptr(fw["mr"]), L.ptr(dx), L.ptr(dres), L.ptr(ws),
                 B, V, C, relu, dt, L.ptr(keep))
            for acc in (0, 1):
                dg, db = (o["dg0"].clone(), o["db0"].clone()) if acc else (nanf(C), nanf(C))
                td, blocks = tail_table(keep, dg, db, B, V, C)
                call(lib, "dreg_bn_param_grad_batched", L.ptr(td), 1, 0, blocks, acc)
                r[f"dgamma{acc}"], r[f"dbeta{acc}"] = dg, db
        torch.cuda.synchronize()
        outs.append(r)
    a, b = outs
    assert torch.isfinite(a["dx"].float()).all() and torch.isfinite(a["dgamma1"]).all()
    for k in a:
        assert torch.equal(a[k], b[k]), f"backward {variant}: {k} differs ({int((a[k] != b[k]).sum())} of {a[k].numel()})"


@pytest.mark.parametrize("case,nch", list(zip(CHUNK_CASES, CHUNKS)), ids=[f"chunks{n}_B{c[0]}" for c, n in zip(CHUNK_CASES, CHUNKS)])
def test_lane_stride_and_grids(case, nch):
    """chunk counts around the 64-lane stride and the tree below it, B = 1 / 3 / 8 / 9; forward and backward variants rotate over the cases"""
    lib = L.load()
    B, V, C, dt = case
    assert lib.dreg_bn_num_chunks(V) == nch
    i = CHUNKS.index(nch)
    o = operands(B, V, C, dt, 100 + i)
    fw = run_forward(lib, B, V, C, dt, FWD_VARIANTS[i % 4], o)
    fw2 = run_forward(lib, B, V, C, dt, FWD_VARIANTS[(i + 2) % 4], o)
    run_backward(lib, B, V, C, dt, BWD_VARIANTS[i % 4], o, fw)
    run_backward(lib, B, V, C, dt, BWD_VARIANTS[(i + 2) % 4], o, fw2)


@pytest.mark.parametrize("case", WIDTH_CASES, ids=[f"B{c[0]}_V{c[1]}_C{c[2]}_{'bf16' if c[3] == 0 else 'fp32'}" for c in WIDTH_CASES])
def test_channel_slabs_all_variants(case):
    """one granule column set, the 128-channel bound, ragged last slabs and a ragged last row block: every forward and backward variant"""
    lib = L.load()
    B, V, C, dt = case
    o = operands(B, V, C, dt, 7 * C + B)
    if (V, C) == (1248, 264):
        rows = lib.dreg_bn_self_coef_rows(B, V, C, dt)
        assert rows == 128 and V % rows != 0
    fws = {v: run_forward(lib, B, V, C, dt, v, o) for v in FWD_VARIANTS}
    for v, f in zip(BWD_VARIANTS, ("relu", "res", "res", "plain")):
        run_backward(lib, B, V, C, dt, v, o, fws[f])


def test_refusals_and_predicate():
    lib = L.load()
    sup, use = lib.dreg_bn_self_coef_supported, lib.dreg_bn_self_coef_use
    assert sup(8, 32768, 1536, 1) == 0           # more than 256 granules, last slab of the statistics pass not full
    assert sup(8, 512, 64, 0) == 0 and use(8, 512, 64, 0, 0) == 0 and use(8, 512, 64, 0, 1) == 0      # the one-launch small form
    assert sup(8, 1, 8, 0) == 0 and sup(257, 1024, 8, 0) == 0 and sup(8, 1024, 12, 0) == 0
    for V, C in ((32768, 64), (32768, 128), (32768, 256), (4096, 128), (4096, 256), (4096, 512)):
        assert sup(8, V, C, 0) == 1
        for bwd in (0, 1):
            assert use(8, V, C, 0, bwd) in (0, 1)
    # a refused shape launches nothing and the three-launch form still runs it
    B, V, C, dt = 2, 64, 64, 0
    o = operands(B, V, C, dt, 5)
    y, ss, mr, keep = nanf(B, V, C, dtype=BF), nanf(B, C, 2), nanf(B, C, 2), nanf(B, C, 2, dtype=torch.float64)
    ws = torch.zeros(B * lib.dreg_bn_num_chunks(V) * C * 2, device=DEV)
    rc = lib.dreg_bn3d_fwd_self_coef(L.ptr(o["x"]), None, L.ptr(y), L.ptr(o["gamma"]), L.ptr(o["beta"]), L.ptr(ss), L.ptr(mr), L.ptr(ws), 8, B, V, C, EPS, 0, dt,
                                     L.ptr(keep), None, L.stream())
    rc2 = lib.dreg_bn3d_bwd_self_coef(L.ptr(o["x"]), L.ptr(o["dy"]), None, L.ptr(ss), L.ptr(mr), L.ptr(y), None, L.ptr(ws), B, V, C, 0, dt, L.ptr(keep), L.stream())
    assert rc != 0 and rc2 != 0
    torch.cuda.synchronize()
    assert torch.isnan(y.float()).all() and torch.isnan(ss).all() and torch.isnan(keep).all()
    call(lib, "dreg_bn3d_fwd", L.ptr(o["x"]), None, L.ptr(y), L.ptr(o["gamma"]), L.ptr(o["beta"]), L.ptr(o["rm"]), L.ptr(o["rv"]), L.ptr(ss), L.ptr(mr), L.ptr(ws),
         B, V, C, EPS, MOM, 1, 0, dt)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()


def test_executor_option_changes_nothing():
    """One forward + backward of the trunk on a 128^3 shell pair (layer 1 at 32^3 per grid, layer 2 at 16^3: the volumes of the large path) with
    bn_self_coef 0 and 1: the output, every activation slot, every parameter gradient and the running statistics agree bit for bit."""
    from dreg_nerf_amd import synth
    from dreg_nerf_amd.optim import FlatAdamW
    from dreg_nerf_amd.regtr import NeRFRegTr
    from dreg_nerf_amd.trunk_exec import exec_opts
    torch.manual_seed(0)
    m = NeRFRegTr(precision="bf16").to(DEV).train()
    opt = FlatAdamW(list(m.parameters()))
    m.native_trunk = True
    grids = []
    for i in range(2):
        g, _ = synth.shell_grid(128, 5 + i, 0.55, 0.8)
        grids.append(g.permute(3, 2, 0, 1).unsqueeze(0).contiguous().to(DEV))
    x = NeRFRegTr.pack_grids(grids, torch.bfloat16)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    go, seen = None, []
    for flag in (0, 1):
        with exec_opts(bn_self_coef=flag):
            m.__dict__.pop("_trunk_cache", None)
            m.load_state_dict(sd0)
            ops.bump_weight_generation()
            opt.zero_grad()
            m.fpn(x, None)                                  # creates the executor and its arena
            (ex,) = m.__dict__["_trunk_cache"].values()
            torch.cuda.synchronize()
            for s in range(1, len(ex.rec.tensors)):         # slots no launch writes (folded BatchNorm outputs) compare as zeros; the rest of the
                off = ex.lib.dreg_exec_tensor_offset(ex.h, s)   # arena (the uploaded tail / reduce tables among it) stays as the executor left it
                ex.arena[off:off + 2 * int(np.prod(ex.rec.tensors[s]))].zero_()
            m.load_state_dict(sd0)
            ops.bump_weight_generation()
            opt.zero_grad()
            p1 = m.fpn(x, None)
            if go is None:
                go = torch.randn(p1.shape, generator=torch.Generator().manual_seed(1)).to(DEV).bfloat16()
            p1.backward(go)
            torch.cuda.synchronize()
            flags = [ex.lib.dreg_exec_op_bn_self_coef(ex.h, i) for i in range(len(ex.rec.ops))]
            acts = []
            for s in range(1, len(ex.rec.tensors)):
                off = ex.lib.dreg_exec_tensor_offset(ex.h, s)
                n = 2
                for d in ex.rec.tensors[s]:
                    n *= d
                acts.append(ex.arena[off:off + n].clone())
            seen.append((p1.detach().clone(), acts, opt.flat_g.clone(), {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}, flags))
    m.__dict__.pop("_trunk_cache", None)
    (o0, a0, g0, s0, f0), (o1, a1, g1, s1, f1) = seen
    lib = L.load()
    assert not any(f0)
    if any(lib.dreg_bn_self_coef_use(2, V, C, 0, bwd) for V in (32768, 4096) for C in (64, 128, 256, 512) for bwd in (0, 1)):
        assert any(f1), "the predicate admits trunk shapes but no BatchNorm op was flagged"
    assert torch.equal(o0, o1)
    for s, (a, b) in enumerate(zip(a0, a1)):
        assert torch.equal(a, b), f"activation slot {s + 1}"
    assert torch.isfinite(g1).all() and torch.equal(g0, g1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
