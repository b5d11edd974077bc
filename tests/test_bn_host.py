"""The table of tests/bn_cases.py is sound (no GPU): every case reaches the launch form it names, the table covers every branch of
bn3d_fwd_impl / bn3d_bwd_impl, every value of bn_rows_per_chunk from 8 up and every NR, the preconditions under which mean, var_keep,
dbeta, dres and the column sums must be EXACT hold on the reference alone, the ambiguous share is within its cap, and the reference is
torch's BatchNorm in fp64.  Host-only calls of the C ABI, as in tests/test_conv_exact_host.py."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as N
from dreg_nerf_amd import lib as L


@pytest.mark.parametrize("c", N.ALL, ids=lambda c: c.id)
def test_case_reaches_its_path(c):
    lib = L.load()
    small = lib.dreg_bn_small(c.B, c.V, c.C, c.dt)
    regs = lib.dreg_bn_small_in_regs(c.B, c.V, c.C, c.dt)
    rpc = N.rows_per_chunk(c.V)
    assert lib.dreg_bn_num_chunks(c.V) == -(-c.V // rpc)
    assert small == int(N.small_ok(c.B, c.V, c.C, c.dt))
    if c.form in ("eval", "from_sums"):          # these never take the one-launch kernels, whatever the shape: `train && !presummed`
        assert c.path == "three"
        if c.form == "from_sums":
            assert c.V % c.rpc == 0
        return
    assert N.path_of(c.B, c.V, c.C, c.dt) == c.path
    assert small == int(c.path != "three") and regs == int(c.path in ("nr1", "nr8"))
    if c.form in ("splitk",):
        assert regs == 1
    if c.form == "res_ss" or "three" in c.name:
        assert small == 0
    if c.form == "ynull":
        assert c.relu and not c.res
    G = 8 if c.dt == 0 else 4
    CG = c.C // G
    assert c.C % G == 0 and not (CG > 256 and CG % 256)


def test_table_covers_the_dispatch():
    three = [c for c in N.THREE]
    assert {N.rows_per_chunk(c.V) for c in three} == {8, 32, 128, 256, 512}
    assert {c.path for c in N.SMALL} == {"nr0", "nr1", "nr8"}
    for dt in (0, 1):                            # both dtypes, in both families, in all four (res, relu) combinations
        for fam in (N.THREE, N.SMALL):
            assert {(c.res, c.relu) for c in fam if c.dt == dt and c.form == "plain"} == {(a, b) for a in (True, False) for b in (True, False)}
        assert {c.path for c in N.SMALL if c.dt == dt} == {"nr0", "nr1", "nr8"}
    for fam in (N.THREE, N.SMALL):
        assert {"plain", "ynull", "acc"} <= {c.form for c in fam}
    assert {c.path for c in N.TRAIN if c.form == "ynull"} == {"three", "nr0", "nr1", "nr8"}
    assert {c.form for c in N.ALL} == {"plain", "ynull", "acc", "eval", "from_sums", "res_ss", "splitk", "defer"}
    # the edges of the three-kernel form the table names
    def geo(c):
        G = 8 if c.dt == 0 else 4
        CG = c.C // G
        cgs = min(CG, 256)
        rpi, rpc = 256 // cgs, N.rows_per_chunk(c.V)
        return CG, cgs, rpi, rpc, -(-c.V // rpc), c.V % rpc
    gs = [geo(c) + (c,) for c in three]
    assert any(tail and tail % rpi for CG, cgs, rpi, rpc, nch, tail, c in gs)                    # chunk tail
    assert any(rpi * cgs < 256 for CG, cgs, rpi, rpc, nch, tail, c in gs)                        # idle threads (r0 >= rpi)
    assert any(rpi > rpc for CG, cgs, rpi, rpc, nch, tail, c in gs)                              # more row lanes than rows
    assert any(rpc > rpi and (rpc // rpi) % 4 for CG, cgs, rpi, rpc, nch, tail, c in gs)         # u-unroll tail
    assert any(nch > 64 and c.B > 8 for CG, cgs, rpi, rpc, nch, tail, c in gs)                   # finalize lane loop and wave loop wrap
    assert {c.dt for CG, cgs, rpi, rpc, nch, tail, c in gs if CG > 256} == {0, 1}                # a second slab in both dtypes
    assert any(c.V == 513 for c in three)
    assert {c.V for c in N.SMALL} >= {2, 64, 210, 512} and any(c.const for c in N.SMALL)
    assert {c.V for c in N.SPLITK} == {64, 512}
    for grp in N.DEFER:
        assert [c.C for c in grp] == [32, 288, 512] and sum(-(-c.C // 256) for c in grp) == 5


@pytest.mark.parametrize("c", N.ALL, ids=lambda c: c.id)
def test_preconditions_of_exactness(c):
    o = N.operands(c)
    x = o["x"]
    assert torch.equal(N.rounded(x, c.dt), x) and torch.equal(N.rounded(o["dy"], c.dt), o["dy"]) and torch.equal(N.rounded(o["res"], c.dt), o["res"])
    assert N.worst_partial(c) < N.LIMIT
    assert float(o["dy"].abs().max()) * max(c.n32, c.rpc) < N.LIMIT and float(o["dy"].abs().sum(1).max()) * c.B + 50 < N.LIMIT
    if c.form == "splitk":
        for key in ("x", "dy"):
            s = o[key + "_slices"]
            assert torch.equal(s, s.float().double()) and float(s.abs().sum(0).max()) < N.LIMIT
        assert torch.equal(o["x_slices"].sum(0), x)
        big = o["dy_slices"].sum(0)
        assert torch.equal(N.rounded(big, c.dt), o["dy"]) and (c.dt == 1 or float((big != o["dy"]).double().mean()) > 0.02)      # the bf16 rounding bites
    if c.form == "res_ss":
        assert N.worst_partial(c, o["xr"]) < N.LIMIT
    # the double mean and variance round to the same fp32 as an exact-rational evaluation
    mean, var = N.stats(x, c.V)
    s1, s2 = x.sum(1).long(), (x * x).sum(1).long()
    assert torch.equal(s1.double(), x.sum(1))
    pick = torch.randperm(s1.numel(), generator=torch.Generator().manual_seed(1))[:1024].tolist()
    for i in pick:
        a, b2 = int(s1.view(-1)[i]), int(s2.view(-1)[i])
        m = Fraction(a, c.V)
        v = Fraction(b2, c.V) - m * m
        assert np.float32(float(m)) == np.float32(float(mean.view(-1)[i])) and np.float32(float(v)) == np.float32(float(var.view(-1)[i])), (c.name, i)
    for ch in c.const:
        assert not var[:, ch].any() and float(o["beta"][ch].abs()) >= 0.05
    assert float(mean.abs().mean()) > 0.5                         # the mean is not near zero


@pytest.mark.parametrize("c", [c for c in N.ALL if c.form not in ("eval", "from_sums", "res_ss")], ids=lambda c: c.id)
def test_ambiguous_share(c):
    """every case whose backward pass runs (the forward-only forms have no mask to get wrong)"""
    f = N.reference(c)
    share = float(f["amb"].double().mean())
    assert share <= N.AMBIGUOUS_CAP, (c.name, int(f["amb"].sum()))
    if c.relu:
        assert 0.1 < float((f["pre"] > 0).double().mean()) < 0.9   # the mask is a real one


def test_reference_is_torch_batchnorm_in_fp64():
    c = next(c for c in N.SMALL if c.name == "small 3x210x64 bf16 res1 relu1")
    o = N.operands(c)
    f = N.forward(c, o["x"], o["gamma"], o["beta"], o["res"])
    bw = N.backward(c, o["x"], o["dy"], f)
    rm_ref, _, rv_ref, _ = N.running(c, f, o["rm0"], o["rv0"])
    xr, rr = o["x"].clone().requires_grad_(True), o["res"].clone().requires_grad_(True)
    ga, be = o["gamma"].clone().requires_grad_(True), o["beta"].clone().requires_grad_(True)
    rm, rv = o["rm0"].clone(), o["rv0"].clone()
    ys = [F.relu(F.batch_norm(xr[b:b + 1].transpose(1, 2), rm, rv, ga, be, True, N.MOM, N.EPS).transpose(1, 2) + rr[b:b + 1]) for b in range(c.B)]
    y = torch.cat(ys)
    y.backward(o["dy"])
    for got, want in ((f["y"], y.detach()), (bw["dx"], xr.grad), (bw["g"], rr.grad), (bw["dgamma"], ga.grad), (bw["dbeta"], be.grad), (rm_ref, rm), (rv_ref, rv)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_column_sum_operands_are_exact():
    for M, C, dt in N.COLSUM:
        g, out0 = N.colsum_operand(M, C, "dense")
        assert torch.equal(N.rounded(g, dt), g) and float(g.abs().sum(0).max()) + 100 < N.LIMIT
    lib = L.load()
    for M in (1, 31, 33, 8191, 8193, 500, 1000):
        assert lib.dreg_colsum_rows_per_chunk(M) == N.colsum_rows_per_chunk(M)
    assert N.colsum_rows_per_chunk(8193) == 64 and -(-8193 // 64) == 129
    assert all(C <= 2048 and C % 8 == 0 for _, C, _ in N.COLSUM_BATCHED)


@pytest.mark.parametrize("name,entry,B,V,C,dt", N.EINVAL, ids=lambda v: v.replace(" ", "_").replace(",", "") if isinstance(v, str) and " " in v else None)
def test_refused_shapes_return_einval_before_any_launch(name, entry, B, V, C, dt):
    """no buffer exists here: a refusal that came after a launch would have had to touch the device"""
    dummy = (ctypes.c_float * 4)()
    rc = N.refused_call(L.load(), entry, B, V, C, dt, lambda k: ctypes.addressof(dummy) if k in ("part", "ss2") else None, None)
    assert rc == -1, name
