"""GPU: the max-pool, fused-stem, downsample-sum and trilinear-gather entries of csrc/fpn_ops.hip against the fp64 references of
tests/fpn_sample_cases.py, called through the C ABI (lib.load() / L.ptr).

What must be exact is compared with torch.equal semantics (pooled values, arg-max bytes, integer gradients, the dyadic trilinear geometries);
everything else against the rounding-count bounds of the cases module, which come from the kernels' source lines and the number formats,
never from a GPU result.  Outputs and scratch are NaN (or 0xff bytes, or a sentinel) beforehand, so a value that was never written cannot pass.
Every test prints `RATIO <case> <family> <worst error / bound>`; the largest ratio of each group over the run goes to
profiles/fpn_sample_fp64_ratios.latest.txt (untracked; profiles/fpn_sample_fp64_ratios.txt holds one run's figures)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import bn_cases as N
import fpn_sample_cases as S
from dreg_nerf_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}              # group -> (ratio, case, family)
SENTINEL = 77.0


def TD(dt):
    return BF if dt == 0 else F32


def dev(t, dtype):
    return t.to(dtype).to(DEV).contiguous()


def devi(a, dtype=torch.int32):
    """a numpy integer array (uint32 arrays go over bit for bit as int32) onto the device"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(dtype).to(DEV).contiguous() if a.size else torch.zeros(0, dtype=dtype, device=DEV)


def nanf(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def call(lib, name, *a):
    L.check(getattr(lib, name)(*a, L.stream()), name)


def _write_worst():
    try:
        with open(os.path.join(ROOT, "profiles", "fpn_sample_fp64_ratios.latest.txt"), "w") as fh:
            fh.write("largest |gpu - fp64| / bound per group, tests/test_hip_fpn_sample_fp64.py\n")
            fh.write("".join(f"{g}: {r:.3e} ({case}, {fam})\n" for g, (r, case, fam) in sorted(WORST.items())))
    except OSError:
        pass


class Report:
    """collects the comparisons of one case; done() prints the ratios and fails with all of them when one comparison missed"""

    def __init__(self, c):
        self.c, self.lines, self.bad = c, [], []

    def bounded(self, group, family, got, want, tol):
        got = got.double().cpu().reshape(want.shape)
        tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(want)
        err = (got - want).abs()
        ratio = torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.where(torch.isnan(got), torch.full_like(err, float("inf")), ratio)
        r = float(ratio.max()) if ratio.numel() else 0.0
        self.lines.append(f"RATIO {self.c.id} {family} {r:.4f}")
        if group not in WORST or r > WORST[group][0]:
            WORST[group] = (r, self.c.id, family)
        if not r <= 1.0:
            i = int(ratio.reshape(-1).argmax())
            self.bad.append(f"{family}: worst error / bound {r:.3f} at flat index {i} (got {float(got.reshape(-1)[i])!r}, fp64 {float(want.reshape(-1)[i])!r}, "
                            f"bound {float(tol.reshape(-1)[i]):.3e}); {int((ratio > 1).sum())} of {ratio.numel()} over")

    def exact(self, family, got, want):
        """want: fp64 holding values the output's dtype represents (or an integer tensor); got: the device tensor"""
        got = got.cpu().reshape(want.shape)
        ne = ~(got.double() == want.double())
        self.lines.append(f"EXACT {self.c.id} {family} {int(ne.sum())} of {ne.numel()} differ")
        if ne.any():
            i = int(ne.reshape(-1).double().argmax())
            self.bad.append(f"{family}: {int(ne.sum())} of {ne.numel()} values differ, first at flat index {i} (got {float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r})")

    def same_bits(self, family, a, b):
        same = torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))
        self.lines.append(f"BITS {self.c.id} {family} {'identical' if same else 'DIFFER'}")
        if not same:
            self.bad.append(f"{family}: two runs are not bit-identical")

    def done(self):
        torch.cuda.synchronize()
        print("\n".join(self.lines))
        _write_worst()
        if self.bad:
            pytest.fail(f"{self.c.name} ({getattr(self.c, 'reaches', '')}):\n  " + "\n  ".join(self.bad) + "\n  all families:\n  " + "\n  ".join(self.lines))


# ================================================================================================ 1. max-pool
@pytest.mark.parametrize("c", S.POOL, ids=lambda c: c.id)
def test_maxpool_forward_backward(c):
    lib, o, rep = L.load(), S.pool_operands(c), Report(c)
    Do, Ho, Wo = c.out
    geo = (c.B, c.D, c.H, c.W, Do, Ho, Wo, c.C)
    y64, tap, idx = S.pool_forward(o["x"])
    dx64 = S.pool_backward(o["dy"], idx, c.D, c.H, c.W)
    x, dy = dev(o["x"], TD(c.dt)), dev(o["dy"], TD(c.dt))
    y = nanf(c.B, Do, Ho, Wo, c.C, dtype=TD(c.dt))
    arg = torch.full((c.B, Do, Ho, Wo, c.C), 255, dtype=torch.uint8, device=DEV)
    call(lib, "dreg_maxpool3d_fwd", L.ptr(x), L.ptr(y), L.ptr(arg), *geo, c.dt)
    rep.exact("pooled", y, y64)
    rep.exact("argmax", arg, tap)
    dx = nanf(c.B, c.D, c.H, c.W, c.C, dtype=TD(c.dt))
    call(lib, "dreg_maxpool3d_bwd", L.ptr(dy), L.ptr(arg), L.ptr(dx), *geo, c.dt)
    rep.exact("dx", dx, dx64)
    dx = nanf(c.B, c.D, c.H, c.W, c.C, dtype=TD(c.dt))
    call(lib, "dreg_maxpool3d_bwd_acc", L.ptr(dy), L.ptr(arg), L.ptr(dx), *geo, 0, c.dt)
    rep.exact("dx acc0", dx, dx64)
    dx = dev(o["dx0"], TD(c.dt))
    call(lib, "dreg_maxpool3d_bwd_acc", L.ptr(dy), L.ptr(arg), L.ptr(dx), *geo, 1, c.dt)
    rep.exact("dx acc1", dx, dx64 + o["dx0"])
    rep.done()


# ================================================================================================ 2. fused stem
class Stem:
    """the device buffers of one fused-stem forward"""

    def __init__(self, lib, c, o):
        Do, Ho, Wo = c.out
        self.geo = (c.B, c.D, c.H, c.W, Do, Ho, Wo, c.C)
        self.x = dev(o["x"].reshape(c.B, c.D, c.H, c.W, c.C), BF)
        self.pooled = nanf(c.B, Do, Ho, Wo, c.C, dtype=BF)
        self.arg = torch.full((c.B, Do, Ho, Wo, c.C), 255, dtype=torch.uint8, device=DEV)
        self.gamma, self.beta = dev(o["gamma"], F32), dev(o["beta"], F32)
        self.rm, self.rv = dev(o["rm0"], F32), dev(o["rv0"], F32)
        self.ss, self.mr = nanf(c.B, c.C, 2), nanf(c.B, c.C, 2)
        self.ws = nanf(c.B * lib.dreg_bn_num_chunks(c.V) * c.C * 2)

    def run(self, lib, train, relu):
        call(lib, "dreg_bn_relu_maxpool_fwd", *(L.ptr(t) for t in (self.x, self.pooled, self.arg, self.gamma, self.beta, self.rm, self.rv, self.ss, self.mr, self.ws)),
             *self.geo, N.EPS, N.MOM, int(train), int(relu))


def stem_selection(c, o, b, relu):
    """the restated activation from the DEVICE's scale_shift, its first-maximum pool and the fp32 pre-activation"""
    act, pre = S.stem_activation(o["x"].reshape(c.B, c.D, c.H, c.W, c.C), b.ss.cpu(), relu)
    y64, tap, idx = S.pool_forward(act)
    return y64, tap, idx, pre


@pytest.mark.parametrize("relu", (1, 0), ids=("relu1", "relu0"))
@pytest.mark.parametrize("train", (1, 0), ids=("train1", "train0"))
@pytest.mark.parametrize("c", S.STEM, ids=lambda c: c.id)
def test_fused_stem_forward(c, train, relu):
    lib, o, rep = L.load(), S.stem_operands(c), Report(c)
    bn = c.bn(bool(relu))
    f = (N.forward(bn, o["x"], o["gamma"], o["beta"]) if train
         else N.forward(bn, o["x"], o["gamma"], o["beta"], mean=o["rm0"][None], var=o["rv0"][None]))
    b = Stem(lib, c, o)
    b.run(lib, train, relu)
    # step 1: the statistics against fp64, with bn_cases' bounds for the three-kernel form
    rep.exact("mean", b.mr[..., 0], f["mean"].float().double())
    rep.bounded("stem stats", "rstd", b.mr[..., 1], f["rstd"], f["rstd_tol"])
    rep.bounded("stem stats", "scale", b.ss[..., 0], f["sc"], f["sc_tol"])
    rep.bounded("stem stats", "shift", b.ss[..., 1], f["sh"], f["sh_tol"])
    if train:
        rm, rm_tol, rv, rv_tol = N.running(bn, f, o["rm0"], o["rv0"])
        rep.bounded("stem stats", "running_mean", b.rm, rm, rm_tol)
        rep.bounded("stem stats", "running_var", b.rv, rv, rv_tol)
    else:
        rep.exact("running_mean untouched", b.rm, o["rm0"])
        rep.exact("running_var untouched", b.rv, o["rv0"])
    # step 2: the selection, exactly, from the device's own scale and shift
    y64, tap, _, _ = stem_selection(c, o, b, relu)
    rep.exact("pooled", b.pooled, y64)
    rep.exact("argmax", b.arg, tap)
    rep.done()


@pytest.mark.parametrize("acc", (0, 1), ids=("acc0", "acc1"))
@pytest.mark.parametrize("relu", (1, 0), ids=("relu1", "relu0"))
@pytest.mark.parametrize("c", S.STEM, ids=lambda c: c.id)
def test_fused_stem_backward(c, relu, acc):
    lib, o, rep = L.load(), S.stem_operands(c), Report(c)
    b = Stem(lib, c, o)
    b.run(lib, 1, relu)
    _, tap, idx, pre = stem_selection(c, o, b, relu)
    rep.exact("argmax", b.arg, tap)
    dy64 = S.pool_backward(o["dp"], idx, c.D, c.H, c.W)
    if relu:
        dy64 = dy64 * (pre > 0)
    dy64 = dy64.reshape(c.B, c.V, c.C)
    bn0 = c.bn(False)                            # the mask is applied above, by the kernel's own expression: nothing left ambiguous
    f0 = N.forward(bn0, o["x"], o["gamma"], o["beta"])
    ref = N.backward(bn0, o["x"], dy64, f0, bool(acc), o["dgamma0"], o["dbeta0"])
    assert bool(ref["dbeta_exact"].all()) and float(dy64.abs().sum(1).max()) * c.B + 50 < N.LIMIT
    dp = dev(o["dp"], BF)
    dx = nanf(c.B, c.V, c.C, dtype=BF)
    dgamma = dev(o["dgamma0"], F32) if acc else nanf(c.C)
    dbeta = dev(o["dbeta0"], F32) if acc else nanf(c.C)
    coef = nanf(c.B, c.C, 2)
    ws = nanf(c.B * lib.dreg_bn_num_chunks(c.V) * c.C * 2)
    call(lib, "dreg_bn_relu_maxpool_bwd", *(L.ptr(t) for t in (b.x, dp, b.arg, b.ss, b.mr, dx, dgamma, dbeta, coef, ws)), *b.geo, int(relu), int(acc))
    rep.exact("dbeta", dbeta, ref["dbeta"])
    rep.bounded("stem dgamma", "dgamma", dgamma, ref["dgamma"], ref["dgamma_tol"])
    rep.bounded("stem dx, bf16", "dx", dx, ref["dx"], ref["dx_tol"])
    rep.done()


# ================================================================================================ 3. downsample-sum
@pytest.mark.parametrize("c", S.DOWN, ids=lambda c: c.id)
def test_downsample_sum_dense_and_rows(c):
    lib, rep = L.load(), Report(c)
    g64 = S.down_operands(c)
    want = S.down_reference(c, g64)
    g = dev(g64, TD(c.dt))
    out = nanf(*want.shape, dtype=TD(c.dt))
    call(lib, "dreg_downsample_sum", L.ptr(g), L.ptr(out), c.B, *c.fine, *c.coarse, c.C, c.dt)
    rep.exact("dense", out, want)
    for kind in S.ROW_LISTS:
        rows = S.down_rows(c, kind)
        exp = torch.full_like(want, S.DOWN_SENTINEL).reshape(-1, c.C)
        exp[torch.from_numpy(rows).long()] = want.reshape(-1, c.C)[torch.from_numpy(rows).long()]
        out = torch.full(want.shape, S.DOWN_SENTINEL, dtype=TD(c.dt), device=DEV)
        rw = devi(rows)
        call(lib, "dreg_downsample_sum_rows", L.ptr(g), L.ptr(out), L.ptr(rw) if len(rows) else None, len(rows), *c.fine, *c.coarse, c.C, c.dt)
        rep.exact(f"rows {kind}", out, exp.reshape(want.shape))
    rep.done()


# ================================================================================================ 4. trilinear gather
class Tri:
    """the device side of one trilinear case"""

    def __init__(self, c, o=None, geom=None):
        self.c = c
        self.geom = geom if geom is not None else o["geom"]
        g = self.geom
        self.N = len(g.idx)
        self.idx, self.ptb = devi(g.idx, torch.int64), devi(g.pt_batch)
        self.rows1, self.map1 = devi(g.rows1), devi(g.map1)
        self.n1 = len(g.rows1)
        self.dims = (*c.coarse, c.C, *c.fine)                     # d, h, w, C, Zr, Xr, Yr
        self.Vf = c.fine[0] * c.fine[1] * c.fine[2]

    def fine_map(self):
        return torch.full((self.c.B * self.Vf,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)

    def dense(self, dt, fill=float("nan")):
        return torch.full((self.geom.nrows, self.c.C), fill, dtype=TD(dt), device=DEV)

    def outside_rows(self):
        m = torch.ones(self.geom.nrows, dtype=torch.bool)
        m[torch.from_numpy(self.geom.rows1).long()] = False
        return m


def seg_device(o, B):
    """(per-pair device tensors kept alive, descs int64 [B][4] on the device): dreg_trilinear_gather_bwd_gather_seg's table"""
    keep, table = [], []
    for p in o["plans"]:
        keep.append((devi(p.inv_seg), dev(torch.from_numpy(p.inv_cnt), F32)))
    for b in range(B):
        p, (iseg, icnt) = o["plans"][b // 2], keep[b // 2]
        table.append([iseg.data_ptr(), icnt.data_ptr(), p.point_start, p.row_off])
    return keep, torch.tensor(table, dtype=torch.int64).to(DEV)


@pytest.mark.parametrize("c", S.TRI, ids=lambda c: c.id)
def test_trilinear_forward_forms(c):
    lib, o, rep = L.load(), S.tri_operands(c), Report(c)
    t = Tri(c, o)
    ref = {dt: S.tri_forward(t.geom, o["p1"][dt]) for dt in (0, 1)}
    for form, dt, odt in (("fwd bf16->fp32", 0, 1), ("fwd bf16->bf16", 0, 0), ("fwd fp32->fp32", 1, 1)):
        if form not in c.insts:
            continue
        out64, mag = ref[dt]
        p1 = dev(o["p1"][dt], TD(dt))
        out = nanf(t.N, c.C, dtype=TD(odt))
        call(lib, "dreg_trilinear_gather_fwd", L.ptr(p1), L.ptr(t.idx), L.ptr(t.ptb), L.ptr(out), t.N, *t.dims, dt, int(odt == 1))
        if c.exact:
            rep.exact(form, out, S.rounded(out64, odt))
        else:
            rep.bounded(f"tri fwd, {S.dt_name(odt)} out", form, out, out64, S.g_(8) * mag + (S.BFU * out64.abs() if odt == 0 else 0.0))
    for form, dt in (("segmean bf16", 0), ("segmean fp32", 1)):
        if form not in c.insts:
            continue
        out64, mag = ref[dt]
        p1 = dev(o["p1"][dt], TD(dt))
        for k, p in enumerate(o["plans"]):
            mean64, m, cnt = S.tri_segment_mean(p, out64, mag)
            order, starts = devi(p.order), devi(p.starts)
            nseg = torch.tensor([p.nseg], dtype=torch.int32).to(DEV)
            out = nanf(p.nseg + 2, c.C)                           # two rows beyond *n_out: they stay untouched
            call(lib, "dreg_gather_segment_mean", L.ptr(p1), L.ptr(t.idx), L.ptr(t.ptb), p.point_start, L.ptr(order), L.ptr(starts), L.ptr(nseg),
                 L.ptr(out), p.nseg + 2, *t.dims, dt)
            assert bool(torch.isnan(out[p.nseg:]).all())
            if c.exact:
                rep.exact(f"{form} pair {k}", out[:p.nseg], mean64)
            else:
                n = 8 + cnt - 1 + 2
                rep.bounded("tri segmean", f"{form} pair {k}", out[:p.nseg], mean64, (n * S.U / (1 - n * S.U))[:, None] * m)
    rep.done()


@pytest.mark.parametrize("c", S.TRI, ids=lambda c: c.id)
def test_trilinear_backward_forms(c):
    lib, o, rep = L.load(), S.tri_operands(c), Report(c)
    t = Tri(c, o)
    geom = t.geom
    dfeat64 = o["dfeat"]
    back = S.tri_backward(geom, dfeat64)
    dfeat = dev(dfeat64, F32)
    outside = t.outside_rows()
    head = (L.ptr(dfeat), L.ptr(t.idx), L.ptr(t.ptb))

    def check(group, family, got, refs, dt, seg=False, gather=False, sentinel=False):
        dp64 = refs[0]
        if sentinel:                             # rows-only form: what was there outside the rows is still there
            rep.exact(f"{family} sentinel", got[outside.to(DEV)], torch.full((int(outside.sum()), c.C), SENTINEL, dtype=torch.float64))
            keep = (~outside).double()[:, None]
            got = torch.where((~outside).to(DEV)[:, None], got, torch.zeros_like(got))
            refs = tuple(r * (keep if r.dim() == 2 else keep[:, 0]) for r in refs)
            dp64 = refs[0]
        if c.exact:
            rep.exact(family, got, S.rounded(dp64, dt))
        else:
            rep.bounded(f"{group}, {S.dt_name(dt)} dp1", family, got, dp64, S.tri_backward_bound(*refs, dt, seg=seg, gather=gather))

    if "bwd atomic fp32" in c.insts:
        dp = torch.zeros(geom.nrows, c.C, dtype=F32, device=DEV)
        call(lib, "dreg_trilinear_gather_bwd", *head, L.ptr(dp), t.N, *t.dims)
        check("tri bwd atomic", "bwd atomic fp32", dp, back, 1)
    for dt in (0, 1):
        if f"bwd_rows {S.dt_name(dt)}" in c.insts:
            comp, dp = nanf(t.n1, c.C), t.dense(dt)
            call(lib, "dreg_trilinear_gather_bwd_rows", *head, L.ptr(t.rows1), t.n1, L.ptr(t.map1), L.ptr(comp), L.ptr(dp), t.N, c.B, *t.dims, dt)
            check("tri bwd rows", f"bwd_rows {S.dt_name(dt)}", dp, back, dt)      # a zero bound outside the rows: they must hold exactly 0
        cpl = c.C // 64
        if f"gather {S.dt_name(dt)} CPL{cpl}" in c.insts:
            fam = f"gather {S.dt_name(dt)} CPL{cpl}"
            runs = []
            for _ in range(2):
                dp = t.dense(dt)
                call(lib, "dreg_trilinear_gather_bwd_gather", *head, L.ptr(t.rows1), t.n1, L.ptr(t.fine_map()), L.ptr(dp), t.N, c.B, *t.dims, dt)
                runs.append(dp)
            check("tri bwd gather", fam, runs[0], back, dt, gather=True)
            rep.same_bits(fam + " run twice", runs[0], runs[1])
            dp = t.dense(dt, SENTINEL)
            call(lib, "dreg_trilinear_gather_bwd_gather_rows_only", *head, L.ptr(t.rows1), t.n1, L.ptr(t.fine_map()), L.ptr(dp), t.N, c.B, *t.dims, dt)
            check("tri bwd gather", fam + " rows_only", dp, back, dt, gather=True, sentinel=True)
            rep.same_bits(fam + " rows_only equals the zero-filling form on the rows", dp[(~outside).to(DEV)], runs[0][(~outside).to(DEV)])
        if f"gather_seg {S.dt_name(dt)} CPL{cpl}" in c.insts:
            fam = f"gather_seg {S.dt_name(dt)} CPL{cpl}"
            g1 = dev(o["g1"], F32)
            keep, descs = seg_device(o, c.B)
            sback = S.tri_backward(geom, S.seg_dfeat(o["plans"], o["g1"], t.N))
            runs = []
            for zero_dense in (1, 1, 0):
                dp = t.dense(dt) if zero_dense else t.dense(dt, SENTINEL)
                call(lib, "dreg_trilinear_gather_bwd_gather_seg", L.ptr(g1), L.ptr(descs), L.ptr(t.idx), L.ptr(t.ptb), L.ptr(t.rows1), t.n1, L.ptr(t.fine_map()),
                     L.ptr(dp), t.N, c.B, *t.dims, dt, zero_dense)
                runs.append(dp)
            check("tri bwd gather seg", fam, runs[0], sback, dt, seg=True, gather=True)
            rep.same_bits(fam + " run twice", runs[0], runs[1])
            check("tri bwd gather seg", fam + " zero_dense 0", runs[2], sback, dt, seg=True, gather=True, sentinel=True)
            del keep
    rep.done()


def test_bracket_sweep_of_the_gather_backward():
    """tri_range and the multi-round candidate loop: one axis varies, every fine voxel occupied, every coarse voxel a row (C = 64, fp32)"""
    lib = L.load()
    rep = Report(dataclasses.replace(S.sweep_case(0, 1, 1), label="sweep"))
    worst = {}
    for axis, n_out, n_in in S.SWEEP:
        c = S.sweep_case(axis, n_out, n_in)
        geom, g64 = S.sweep_operands(c)
        t = Tri(c, geom=geom)
        refs = S.tri_backward(geom, g64)
        g = dev(g64, F32)
        dp = t.dense(1)
        call(lib, "dreg_trilinear_gather_bwd_gather", L.ptr(g), L.ptr(t.idx), L.ptr(t.ptb), L.ptr(t.rows1), t.n1, L.ptr(t.fine_map()), L.ptr(dp),
             t.N, 1, *t.dims, 1)
        rep.c = dataclasses.replace(c, label=f"sweep axis {axis}")
        rep.bounded("tri bracket sweep", f"{n_out}<-{n_in}", dp, refs[0], S.tri_backward_bound(*refs, 1, gather=True))
        worst[axis] = max(worst.get(axis, 0.0), float(rep.lines.pop().rsplit(" ", 1)[1]))
    rep.lines = [f"RATIO sweep axis {a} {len([s for s in S.SWEEP if s[0] == a])} pairs {r:.4f}" for a, r in sorted(worst.items())]
    rep.done()


# ================================================================================================ 5. empty inputs
def test_empty_inputs_write_what_they_promise_and_nothing_else():
    lib = L.load()
    c = S.TRI_EXACT[0]
    o = S.tri_operands(c)
    t = Tri(c, o)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    for dt in (0, 1):
        p1 = dev(o["p1"][dt], TD(dt))
        out = nanf(4, c.C)
        call(lib, "dreg_trilinear_gather_fwd", L.ptr(p1), None, None, L.ptr(out), 0, *t.dims, dt, 1)
        assert bool(torch.isnan(out).all())
        call(lib, "dreg_gather_segment_mean", L.ptr(p1), None, None, 0, None, None, None, L.ptr(out), 0, *t.dims, dt)      # M = 0
        assert bool(torch.isnan(out).all())
        dfeat = dev(o["dfeat"], F32)
        for N_, n1 in ((0, t.n1), (t.N, 0), (0, 0)):
            head = (L.ptr(dfeat) if N_ else None, L.ptr(t.idx) if N_ else None, L.ptr(t.ptb) if N_ else None, L.ptr(t.rows1) if n1 else None, n1)
            dp = t.dense(dt)
            call(lib, "dreg_trilinear_gather_bwd_rows", *head, L.ptr(t.map1), None, L.ptr(dp), N_, c.B, *t.dims, dt)
            assert float(dp.float().abs().max()) == 0.0
            dp = t.dense(dt)
            call(lib, "dreg_trilinear_gather_bwd_gather", *head, None, L.ptr(dp), N_, c.B, *t.dims, dt)
            assert float(dp.float().abs().max()) == 0.0                  # the dense buffer is zero-filled although nothing is gathered
            dp = t.dense(dt, SENTINEL)
            call(lib, "dreg_trilinear_gather_bwd_gather_rows_only", *head, None, L.ptr(dp), N_, c.B, *t.dims, dt)
            assert bool((dp.float() == SENTINEL).all())
    dp = torch.zeros(8, c.C, dtype=F32, device=DEV)
    call(lib, "dreg_trilinear_gather_bwd", None, None, None, L.ptr(dp), 0, *t.dims)
    assert float(dp.abs().max()) == 0.0 and none.numel() == 0
    torch.cuda.synchronize()
