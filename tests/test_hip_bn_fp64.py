"""GPU: every BatchNorm launch form and every column-sum form of csrc/fpn_ops.hip on the integer operands of tests/bn_cases.py against fp64.

What must be exact is compared with torch.equal (the per-grid mean, var_keep, dbeta, dres, the x a split-K forward writes back, every column
sum); everything else against the rounding-count bounds derived in the docstring of tests/bn_cases.py, which come from the kernels' source
lines and the number formats, never from a GPU result.  Outputs and workspaces are NaN beforehand, so a value that was never written cannot
pass.  Every test prints `RATIO <case> <family> <worst error / bound>`; a failure lists the worst ratio of each family of the case."""
import ctypes

import numpy as np
import pytest
import torch

import bn_cases as N
from dreg_nerf_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF, F32 = torch.bfloat16, torch.float32
TAIL_DT = np.dtype([("a", "<u8"), ("b", "<u8"), ("o0", "<u8"), ("o1", "<u8"), ("B", "<i4"), ("V", "<i4"), ("C", "<i4"), ("block0", "<i4")])
COLSUM_DT = np.dtype([("g", "<u8"), ("out", "<u8"), ("partial", "<u8"), ("M", "<i4"), ("C", "<i4"), ("rpc", "<i4"), ("nch", "<i4"),
                      ("pblock0", "<i4"), ("fblock0", "<i4"), ("accumulate", "<i4"), ("pad", "<i4")])
assert TAIL_DT.itemsize == 48 and COLSUM_DT.itemsize == 56


def T(c):
    return BF if c.dt == 0 else F32


def dev(t, dtype):
    return t.to(dtype).to(DEV).contiguous()


def nanf(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def call(lib, name, *a):
    L.check(getattr(lib, name)(*a, L.stream()), name)


class Report:
    """collects the comparisons of one case; done() prints the ratios and fails with all of them when one comparison missed"""

    def __init__(self, c):
        self.c, self.lines, self.bad = c, [], []

    def bounded(self, family, got, want, tol, keep=None):
        got = got.double().cpu().reshape(want.shape)
        err = (got - want).abs()
        ratio = torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.where(torch.isnan(got), torch.full_like(err, float("inf")), ratio)
        if keep is not None:
            ratio = torch.where(keep.expand_as(ratio), ratio, torch.zeros_like(ratio))
        r = float(ratio.max())
        self.lines.append(f"RATIO {self.c.id} {family} {r:.4f}")
        if not r <= 1.0:
            i = int(ratio.reshape(-1).argmax())
            self.bad.append(f"{family}: worst error / bound {r:.3f} at flat index {i} (got {float(got.reshape(-1)[i])!r}, fp64 {float(want.reshape(-1)[i])!r}, "
                            f"bound {float(tol.reshape(-1)[i]):.3e}); {int((ratio > 1).sum())} of {ratio.numel()} over")

    def exact(self, family, got, want, keep=None):
        """want: fp64 holding values the output's dtype represents; got: the device tensor"""
        got = got.cpu().reshape(want.shape)
        ne = ~(got.double() == want)
        if keep is not None:
            ne &= keep
        self.lines.append(f"EXACT {self.c.id} {family} {int(ne.sum())} of {ne.numel()} differ")
        if ne.any():
            i = int(ne.reshape(-1).double().argmax())
            self.bad.append(f"{family}: {int(ne.sum())} of {ne.numel()} values differ, first at flat index {i} (got {float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r})")

    def done(self):
        torch.cuda.synchronize()
        print("\n".join(self.lines))
        if self.bad:
            pytest.fail(f"{self.c.name} ({self.c.reaches or self.c.form}):\n  " + "\n  ".join(self.bad) + "\n  all families:\n  " + "\n  ".join(self.lines))


class Fwd:
    """the device buffers of one forward call"""

    def __init__(self, lib, c, o, x=None, res=None, gamma="gamma", beta="beta", with_y=True):
        B, V, C = c.B, c.V, c.C
        self.x = dev(o["x"], T(c)) if x is None else x
        self.res = (dev(o["res"], T(c)) if c.res else None) if res is None else res
        self.y = nanf(B, V, C, dtype=T(c)) if with_y else None
        self.gamma, self.beta = dev(o[gamma], F32), dev(o[beta], F32)
        self.rm, self.rv = dev(o["rm0"], F32), dev(o["rv0"], F32)
        self.ss, self.mr = nanf(B, C, 2), nanf(B, C, 2)
        self.ws = nanf(max(B * lib.dreg_bn_num_chunks(V) * C * 2, B * C))

    def head(self):
        return tuple(L.ptr(t) for t in (self.x, self.res, self.y, self.gamma, self.beta, self.rm, self.rv, self.ss, self.mr))


def check_forward(rep, c, f, b, o, run_stats=True, y=True):
    rep.exact("mean", b.mr[..., 0], f["mean"].float().double())
    rep.bounded("rstd", b.mr[..., 1], f["rstd"], f["rstd_tol"])
    rep.bounded("scale", b.ss[..., 0], f["sc"], f["sc_tol"])
    rep.bounded("shift", b.ss[..., 1], f["sh"], f["sh_tol"])
    if y:
        rep.bounded("y", b.y, f["y"], f["y_tol"])
    if run_stats:
        rm, rm_tol, rv, rv_tol = N.running(c, f, o["rm0"], o["rv0"])
        rep.bounded("running_mean", b.rm, rm, rm_tol)
        rep.bounded("running_var", b.rv, rv, rv_tol)


class Bwd:
    def __init__(self, lib, c, o, fw, accumulate, y_null=False, dy=True):
        B, V, C = c.B, c.V, c.C
        self.dy = dev(o["dy"], T(c)) if dy else None
        self.y = None if y_null else fw.y
        self.dx = nanf(B, V, C, dtype=T(c))
        self.dres = nanf(B, V, C, dtype=T(c)) if c.res else None
        self.dgamma = dev(o["dgamma0"], F32) if accumulate else nanf(C)
        self.dbeta = dev(o["dbeta0"], F32) if accumulate else nanf(C)
        self.coef = nanf(B, C, 2)
        self.ws = nanf(max(B * lib.dreg_bn_num_chunks(V) * C * 2, B * C))
        self.fw = fw

    def head(self):
        return tuple(L.ptr(t) for t in (self.fw.x, self.dy, self.y, self.fw.ss, self.fw.mr, self.dx, self.dres, self.dgamma, self.dbeta, self.coef, self.ws))


def check_backward(rep, c, bw, b, params=True):
    if params:
        rep.exact("dbeta", b.dbeta, bw["dbeta"], keep=bw["dbeta_exact"])
        rep.bounded("dgamma", b.dgamma, bw["dgamma"], bw["dgamma_tol"])
    if b.dres is not None:
        rep.exact("dres", b.dres, bw["g"], keep=bw["keep"])
    rep.bounded("dx", b.dx, bw["dx"], bw["dx_tol"], keep=bw["keep"])


# ------------------------------------------------------------------------------------------------ training mode, both path families
@pytest.mark.parametrize("c", N.TRAIN, ids=lambda c: c.id)
def test_train_forward_backward(c):
    """dreg_bn3d_fwd, then dreg_bn3d_bwd on what it saved: (res, relu) combinations, y == NULL, accumulate"""
    lib, o, rep = L.load(), N.operands(c), Report(c)
    f = N.reference(c)
    fw = Fwd(lib, c, o)
    call(lib, "dreg_bn3d_fwd", *fw.head(), L.ptr(fw.ws), c.B, c.V, c.C, N.EPS, N.MOM, 1, int(c.relu), c.dt)
    check_forward(rep, c, f, fw, o)
    acc = c.form == "acc"
    ref = N.backward(c, o["x"], o["dy"], f, acc, o["dgamma0"], o["dbeta0"])
    bw = Bwd(lib, c, o, fw, acc, y_null=c.form == "ynull")
    call(lib, "dreg_bn3d_bwd", *bw.head(), c.B, c.V, c.C, int(c.relu), int(acc), c.dt)
    check_backward(rep, c, ref, bw)
    rep.done()


@pytest.mark.parametrize("c", N.EVAL, ids=lambda c: c.id)
def test_eval_forward(c):
    lib, o, rep = L.load(), N.operands(c), Report(c)
    f = N.reference(c)
    fw = Fwd(lib, c, o)
    call(lib, "dreg_bn3d_fwd", *fw.head(), L.ptr(fw.ws), c.B, c.V, c.C, N.EPS, N.MOM, 0, int(c.relu), c.dt)
    check_forward(rep, c, f, fw, o, run_stats=False)
    rep.exact("running_mean untouched", fw.rm, o["rm0"])
    rep.exact("running_var untouched", fw.rv, o["rv0"])
    rep.done()


@pytest.mark.parametrize("c", N.FROM_SUMS, ids=lambda c: c.id)
def test_forward_from_chunk_sums(c):
    """dreg_bn3d_fwd_from_sums: finalize and apply only, from chunk sums formed here"""
    lib, o, rep = L.load(), N.operands(c), Report(c)
    f = N.reference(c)
    fw = Fwd(lib, c, o)
    sums = dev(N.chunk_sums(o["x"], c.rpc), F32)
    assert torch.equal(sums.double().cpu(), N.chunk_sums(o["x"], c.rpc))
    call(lib, "dreg_bn3d_fwd_from_sums", *fw.head(), L.ptr(sums), c.rpc, c.B, c.V, c.C, N.EPS, N.MOM, int(c.relu), c.dt)
    check_forward(rep, c, f, fw, o)
    rep.done()


@pytest.mark.parametrize("c", N.RES_SS, ids=lambda c: c.id)
def test_residual_from_an_unapplied_batchnorm(c):
    """dreg_bn3d_fwd_ex with y = NULL on the branch, then the consumer given res_scale_shift: against fp64, and bit for bit against the branch
    applied on its own and handed over as a stored residual (the fp64 bound cannot see a missing bf16 rounding of the residual: it only helps)"""
    lib, o, rep = L.load(), N.operands(c), Report(c)
    B, V, C = c.B, c.V, c.C
    geo = (B, V, C, N.EPS, N.MOM, 1)
    xr = dev(o["xr"], T(c))
    branch = N.Case(c.name + " branch", B, V, C, c.dt, "three", res=False, relu=False)
    fb = N.forward(branch, o["xr"], o["gamma_r"], o["beta_r"])
    a = Fwd(lib, branch, o, x=xr, gamma="gamma_r", beta="beta_r", with_y=False)
    call(lib, "dreg_bn3d_fwd_ex", *a.head(), L.ptr(a.ws), *geo, 0, c.dt, None, None, 0, None)
    brep = Report(branch)
    check_forward(brep, branch, fb, a, o, y=False)
    brep.done()
    fw = Fwd(lib, c, o, res=xr)
    ex = N.BnExtra(L.ptr(a.ss), None, 0, 0)
    call(lib, "dreg_bn3d_fwd_ex", *fw.head(), L.ptr(fw.ws), *geo, int(c.relu), c.dt, None, None, 0, ctypes.addressof(ex))
    check_forward(rep, c, N.reference(c), fw, o)
    # the same in two steps: the branch applied and stored, then a plain residual
    a2 = Fwd(lib, branch, o, x=xr, gamma="gamma_r", beta="beta_r")
    call(lib, "dreg_bn3d_fwd", *a2.head(), L.ptr(a2.ws), *geo, 0, c.dt)
    r64, R = N.unapplied_residual(c, o["xr"], o["gamma_r"], o["beta_r"])
    rep.bounded("branch y", a2.y, r64, R)
    fw2 = Fwd(lib, c, o, res=a2.y)
    call(lib, "dreg_bn3d_fwd", *fw2.head(), L.ptr(fw2.ws), *geo, int(c.relu), c.dt)
    rep.exact("y, folded against two steps", fw.y, fw2.y.double().cpu())
    rep.done()


@pytest.mark.parametrize("c", N.SPLITK, ids=lambda c: c.id)
def test_splitk_slices_summed_in_the_kernel(c):
    """dreg_bn_extra.splitk_part: the forward's x and the backward's dy arrive as three fp32 slices"""
    lib, o, rep = L.load(), N.operands(c), Report(c)
    B, V, C = c.B, c.V, c.C
    assert lib.dreg_bn_small_in_regs(B, V, C, c.dt) == 1
    f = N.reference(c)
    fw = Fwd(lib, c, o, x=nanf(B, V, C, dtype=T(c)))
    xs = dev(o["x_slices"], F32)
    ex = N.BnExtra(None, L.ptr(xs), 3, B * V * C)
    call(lib, "dreg_bn3d_fwd_ex", *fw.head(), L.ptr(fw.ws), B, V, C, N.EPS, N.MOM, 1, int(c.relu), c.dt, None, None, 0, ctypes.addressof(ex))
    rep.exact("x written back", fw.x, N.rounded(o["x_slices"].sum(0), c.dt))
    check_forward(rep, c, f, fw, o)
    ref = N.backward(c, o["x"], o["dy"], f)
    bw = Bwd(lib, c, o, fw, False, dy=False)
    gs = dev(o["dy_slices"], F32)
    ex = N.BnExtra(None, L.ptr(gs), 3, B * V * C)
    call(lib, "dreg_bn3d_bwd_ex", *bw.head(), B, V, C, int(c.relu), 0, c.dt, None, None, ctypes.addressof(ex))
    check_backward(rep, c, ref, bw)
    rep.done()


def _tail_table(rows):
    """rows: (a, b, o0, o1, case) -> the device table of BnTailDesc records and the number of 256-channel workgroups"""
    table, blocks = np.zeros(len(rows), dtype=TAIL_DT), 0
    for i, (a, b, o0, o1, c) in enumerate(rows):
        table[i] = (a.data_ptr(), 0 if b is None else b.data_ptr(), o0.data_ptr(), o1.data_ptr(), c.B, c.V, c.C, blocks)
        blocks += -(-c.C // 256)
    return torch.from_numpy(table.view(np.uint8)).to(DEV), blocks


@pytest.mark.parametrize("cases", N.DEFER, ids=lambda cs: cs[0].id.split("_")[-1])
def test_deferred_tails(cases):
    """dreg_bn3d_fwd_defer_update + dreg_bn_running_update_batched, dreg_bn3d_bwd_defer_params + dreg_bn_param_grad_batched: three layers,
    each batched tail as two launches split by block_base / nblocks; the parameter gradients with accumulate = 0 and = 1"""
    lib = L.load()
    reps, fwd, bwd, refs = [], [], [], []
    for c in cases:
        o, rep = N.operands(c), Report(c)
        f = N.reference(c)
        fw = Fwd(lib, c, o)
        var_keep, flag = nanf(c.B, c.C), ctypes.c_int(-1)
        call(lib, "dreg_bn3d_fwd_defer_update", *fw.head(), L.ptr(fw.ws), c.B, c.V, c.C, N.EPS, N.MOM, 1, int(c.relu), c.dt, L.ptr(var_keep), ctypes.addressof(flag))
        assert flag.value == 1
        check_forward(rep, c, f, fw, o, run_stats=False)
        rep.exact("var_keep", var_keep, f["var"].float().double())
        rep.exact("running_mean before the tail", fw.rm, o["rm0"])
        rep.exact("running_var before the tail", fw.rv, o["rv0"])
        bw = Bwd(lib, c, o, fw, True)
        sums, flag = nanf(c.B, c.C, 2), ctypes.c_int(-1)
        call(lib, "dreg_bn3d_bwd_defer_params", *bw.head(), c.B, c.V, c.C, int(c.relu), 1, c.dt, L.ptr(sums), ctypes.addressof(flag))
        assert flag.value == 1
        ref = N.backward(c, o["x"], o["dy"], f, True, o["dgamma0"], o["dbeta0"])
        check_backward(rep, c, ref, bw, params=False)
        rep.exact("sums_keep sum g", sums[..., 0], ref["s1"], keep=(~f["amb"]).all(1))
        rep.bounded("sums_keep sum g xhat", sums[..., 1], ref["s2"], ref["s2_tol"])
        rep.exact("dgamma before the tail", bw.dgamma, o["dgamma0"])
        rep.exact("dbeta before the tail", bw.dbeta, o["dbeta0"])
        reps.append(rep), fwd.append((fw, var_keep)), bwd.append((bw, sums)), refs.append((f, ref))
    td, blocks = _tail_table([(fw.mr, vk, fw.rm, fw.rv, c) for (fw, vk), c in zip(fwd, cases)])
    assert blocks == 5
    call(lib, "dreg_bn_running_update_batched", L.ptr(td), 3, 0, 2, N.MOM)
    call(lib, "dreg_bn_running_update_batched", L.ptr(td), 3, 2, 3, N.MOM)
    fresh = [(nanf(c.C), nanf(c.C)) for c in cases]
    t0, _ = _tail_table([(s, None, dg, db, c) for (bw, s), (dg, db), c in zip(bwd, fresh, cases)])
    t1, _ = _tail_table([(s, None, bw.dgamma, bw.dbeta, c) for (bw, s), c in zip(bwd, cases)])
    for table, accumulate in ((t0, 0), (t1, 1)):
        call(lib, "dreg_bn_param_grad_batched", L.ptr(table), 3, 0, 2, accumulate)
        call(lib, "dreg_bn_param_grad_batched", L.ptr(table), 3, 2, 3, accumulate)
    for c, rep, (fw, _), (bw, _), (f, ref), (dg, db) in zip(cases, reps, fwd, bwd, refs, fresh):
        o = N.operands(c)
        rm, rm_tol, rv, rv_tol = N.running(c, f, o["rm0"], o["rv0"])
        rep.bounded("running_mean", fw.rm, rm, rm_tol)
        rep.bounded("running_var", fw.rv, rv, rv_tol)
        plain = N.backward(c, o["x"], o["dy"], f)
        rep.exact("dbeta", db, plain["dbeta"], keep=plain["dbeta_exact"])
        rep.bounded("dgamma", dg, plain["dgamma"], plain["dgamma_tol"])
        rep.exact("dbeta accumulated", bw.dbeta, ref["dbeta"], keep=ref["dbeta_exact"])
        rep.bounded("dgamma accumulated", bw.dgamma, ref["dgamma"], ref["dgamma_tol"])
    for rep in reps:
        rep.done()


# ------------------------------------------------------------------------------------------------ contracts
@pytest.mark.parametrize("name,entry,B,V,C,dt", N.EINVAL, ids=lambda v: v.replace(" ", "_").replace(",", "") if isinstance(v, str) and " " in v else None)
def test_refused_shapes_launch_nothing(name, entry, B, V, C, dt):
    """DREG_EINVAL, and every buffer the call was handed is as it was (all of them NaN, with room to spare: nothing is read or written past a row
    even by a library that did launch)"""
    lib = L.load()
    n = (B * V + 8) * (C + 2048)
    bufs = {}

    def p(k):
        if k in bufs:
            return L.ptr(bufs[k])
        if k == "rows":
            bufs[k] = torch.zeros(V + 8, dtype=torch.int32, device=DEV)
        elif k == "argmax":
            bufs[k] = torch.zeros(n, dtype=torch.uint8, device=DEV)
        elif k in ("x", "res", "y", "dy", "dx", "dres"):
            bufs[k] = nanf(n, dtype=BF if dt == 0 else F32)
        else:
            bufs[k] = nanf(max(3 * n if k == "part" else 2 * n, 4096))
        return L.ptr(bufs[k])
    rc = N.refused_call(lib, entry, B, V, C, dt, p, L.stream())
    torch.cuda.synchronize()
    assert rc == -1, name
    for k, t in bufs.items():
        assert bool(torch.isnan(t).all()) if t.is_floating_point() else not bool(t.any()), (name, k)


# ------------------------------------------------------------------------------------------------ column sums
def _colsum(lib, g, out, M, C, accumulate, dt, rows=None):
    ws = nanf(lib.dreg_colsum_workspace_bytes(M, C) // 4)
    if rows is None:
        call(lib, "dreg_colsum", L.ptr(g), L.ptr(out), L.ptr(ws), M, C, accumulate, dt)
    else:
        call(lib, "dreg_colsum_rows", L.ptr(g), L.ptr(rows), M, L.ptr(out), L.ptr(ws), C, accumulate, dt)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,C,dt", N.COLSUM, ids=lambda v: str(v))
def test_colsum_exact(M, C, dt):
    lib = L.load()
    g, out0 = N.colsum_operand(M, C, "dense")
    gd = dev(g, BF if dt == 0 else F32)
    want = g.sum(0)
    assert torch.equal(_colsum(lib, gd, nanf(C), M, C, 0, dt).cpu(), want.float())
    assert torch.equal(_colsum(lib, gd, dev(out0, F32), M, C, 1, dt).cpu(), (want + out0).float())


@pytest.mark.parametrize("nrows,C,dt", N.COLSUM_ROWS, ids=lambda v: str(v))
def test_colsum_rows_exact(nrows, C, dt):
    lib = L.load()
    g, out0 = N.colsum_operand(500, C, "rows")
    rows = torch.randperm(500, generator=torch.Generator().manual_seed(nrows))[:nrows].sort().values
    want = g[rows].sum(0)
    gd, rd = dev(g, BF if dt == 0 else F32), rows.to(torch.int32).to(DEV)
    assert torch.equal(_colsum(lib, gd, nanf(C), nrows, C, 0, dt, rd).cpu(), want.float())
    assert torch.equal(_colsum(lib, gd, dev(out0, F32), nrows, C, 1, dt, rd).cpu(), (want + out0).float())


def test_colsum_batched_exact():
    """three records of different M and C in one launch pair, mixed accumulate: equal to the fp64 sums and to dreg_colsum record by record"""
    lib = L.load()
    table = np.zeros(len(N.COLSUM_BATCHED), dtype=COLSUM_DT)
    keep, pb, fb = [], 0, 0
    for i, (M, C, acc) in enumerate(N.COLSUM_BATCHED):
        g, out0 = N.colsum_operand(M, C, "batched")
        gd, out = dev(g, BF), (dev(out0, F32) if acc else nanf(C))
        rpc = lib.dreg_colsum_rows_per_chunk(M)
        nch = -(-M // rpc)
        part = nanf(lib.dreg_colsum_workspace_bytes(M, C) // 4)
        table[i] = (gd.data_ptr(), out.data_ptr(), part.data_ptr(), M, C, rpc, nch, pb, fb, acc, 0)
        pb, fb = pb + nch, fb + -(-C // 4)
        keep.append((g, out0, gd, out, part))
    td = torch.from_numpy(table.view(np.uint8)).to(DEV)
    call(lib, "dreg_colsum_batched", L.ptr(td), len(keep), pb, fb)
    torch.cuda.synchronize()
    for (M, C, acc), (g, out0, gd, out, part) in zip(N.COLSUM_BATCHED, keep):
        want = g.sum(0) + (out0 if acc else 0)
        assert torch.equal(out.cpu(), want.float()), (M, C)
        single = _colsum(lib, gd, dev(out0, F32) if acc else nanf(C), M, C, acc, 0)
        assert torch.equal(out, single), (M, C)
