"""The table of tests/conv_exact_cases.py is sound (no GPU): every case reaches the instantiation it names, the default-knob cases cover
what the default build can dispatch, and the preconditions under which an fp32-accumulating kernel must reproduce the fp64 reference
EXACTLY hold on the reference alone.  Host-only calls of the C ABI, as in tests/test_abi_and_ddp.py."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as C
from dreg_nerf_amd import lib as L

FWD_LIKE = C.FWD + C.DGRAD
WG_LIKE = C.WGRAD + [c for _, _, cs in C.GROUPS for c in cs]


def _query(c):
    if not c.knobs:
        return C.variant_query(L.load(), c)
    with L.probe() as p:
        for setter, value, default in c.knobs:
            p.set(setter, value, default)
        return C.variant_query(p.lib, c)


@pytest.mark.parametrize("c", C.ALL, ids=lambda c: c.id)
def test_case_reaches_its_variant(c):
    assert _query(c) == c.variant


def test_group_launches_share_one_tile_shape():
    for name, variant, cases in C.GROUPS:
        assert [_query(c) for c in cases] == [variant] * len(cases), name


def test_split_states():
    """split-K cases really split (a workspace is asked for), the refused ones do not; the row-list partials case writes fewer slices than the
    workspace is sized for (the dense rule's count), which is what its reduce must honour"""
    lib = L.load()
    for c in FWD_LIKE:
        if c.knobs or c.api not in ("fwd", "bnstats", "defer", "dgrad"):
            continue
        geo = (c.B, *c.din, c.cin, *c.dout, c.cout, c.k, c.s, c.p, 0) if c.api != "dgrad" else (c.B, *c.dout, c.cout, *c.din, c.creal, c.k, c.s, c.p, 1)
        nws = lib.dreg_conv3d_igemm_workspace_bytes(*geo, int(bool(c.addend)), c.dt)
        assert (nws > 0) == (c.variant % 10 == 1 or (not c.ws and "no workspace" in c.name)), c.name
    c = next(c for c in C.WGRAD if c.name == "wgrad partials rows fewer slices")
    smax = lib.dreg_conv3d_wgrad_splits(c.B, *c.dout, c.cin, c.cout, c.k, 0)
    assert smax == 4 and -(-len(C.rows(c)) // 1024) == 2          # the four-wave row-list rule: 1,024 rows per split for 3^3 taps
    c = next(c for c in C.WGRAD if "empty last splits" in c.name)
    s = lib.dreg_conv3d_wgrad_splits(c.B, *c.dout, c.cin, c.cout, c.k, 0)
    vps = -(-(-(-c.M // s)) // 64) * 64
    assert (s - 1) * vps >= c.M, "the last split of this case is meant to start past the last row"


def test_default_cases_cover_the_default_dispatch():
    """The codes reached with every knob at its default are exactly the instantiations the default build dispatches; written out so that
    dropping a case fails here.  igemm_glds_dispatch: six of its eight lines are reachable at defaults (x split-K for the 128-row tiles); the
    lockstep 256 x 256 and the 128 x 256 tile exist only behind igemm_ap256 = 0 / glds = 3 and are in the knob set, `dbg` (igemm_probe) is excluded."""
    igemm = {c.variant for c in FWD_LIKE if not c.knobs and c.variant is not None}
    assert igemm == {
        25625610,                                   # 256 x 256 anti-phase
        12812810, 12806410, 12812800, 12806400,     # 128 x {128, 64}, anti-phase and four-wave
        12812811, 12806411, 12812801, 12806401,     # the same four as split-K launches
        112812800, 112806400,                       # register-staged, both widths
    }
    assert {c.variant for c in FWD_LIKE if c.knobs} == {25625600, 12825600, 12812800, 12806400, 112812800}
    wg = {(C.wgrad_kind(c), c.variant) for c in WG_LIKE if not c.knobs and c.variant is not None}
    assert wg == {
        ("dense", 256256),                                                               # WG_DENSE8 (fast loop, general loop, ragged Kpad)
        ("dense", 128128), ("dense", 128064), ("dense", 64128), ("dense", 64064),        # WG_GLDS4, all four tiles
        ("group", 128128), ("group", 128064), ("group", 64128), ("group", 64064),        # the same through the grouped launch
        ("occ", 64064), ("rows", 64064),                                                 # WG_GLDS4 with occupancy flags / on a row list
        ("rows", 256256),                                                                # WG_ROWS8_AP
    }
    # WG_REG at defaults: the fp32 and use_tr = 0 launches (the label function speaks of bf16 / use_tr = 1 only)
    assert sorted(c.name for c in C.WGRAD if not c.knobs and c.variant is None) == ["wgrad bf16 use_tr 0", "wgrad fp32"]
    # (WG_ROWS8 needs a list of >= 65,536 rows whose anti-phase slice does not fit in LDS, WG_256x128 wgrad_big = 1: neither is a default form here)
    assert {(C.wgrad_kind(c), c.variant) for c in WG_LIKE if c.knobs} == {("dense", 1128128), ("dense", 128128), ("dense", 128064), ("dense", 256128), ("dense", 256256),
                                                                          ("rows", 64064), ("rows", 128128), ("rows", 256256)}


@pytest.mark.parametrize("c", C.ALL, ids=lambda c: c.id)
def test_geometry_claims(c):
    """ragged row tiles, pairwise different non-power-of-two output dims, odd dims for the parity-class gradient, Kpad"""
    lib = L.load()
    rows = c.M if c.nrows < 0 else len(C.rows(c))
    if c.ragged:
        assert rows % c.ragged != 0
    if "256x256" in c.name or "dense8" in c.name or c.variant == 256256 and c.nrows < 0:
        assert c.M >= 65536
    if c.api == "dgrad_s2":
        assert all(d % 2 == 1 for d in c.din)
    if c.din in (C.SMALL, C.MID, C.WIDE, C.LONG, C.HUGE, C.ODD):
        do = c.dout
        assert len(set(do)) == 3 and all(d & (d - 1) for d in do)
    if "stem" in c.name:
        assert (c.k, c.s, c.cin, c.creal) == (5, 2, 8, 4) and 125 * 8 == 1000 and lib.dreg_conv3d_kpad(5, 8, 0) == 1024
    if "1728" in c.name:
        assert lib.dreg_conv3d_kpad(c.k, c.cin, 0) == 1728 and 1728 % 256 != 0
    assert C.worst_sum(c) < C.LIMIT


def _frac_unrepresentable(y):
    return float((y.float().bfloat16().double() != y).double().mean())


@pytest.mark.parametrize("c", [c for c in C.ALL + C.HALO + C.BRICK if not c.knobs], ids=lambda c: c.id)
def test_preconditions_of_exactness(c):
    """on the reference alone: enough nonzero outputs, bf16 outputs that need rounding, data on all six faces, BatchNorm sums below 2^24"""
    o = C.operands(c)
    if c.api in ("fwd", "fwd_occ", "rows", "bnstats", "defer", "halo", "brick"):
        y, bf16_out = C.fwd_exact(c), c.dt == 0 and not c.out_f32 and c.api != "defer"
        faces = o.get("x")[..., :c.creal]
    elif c.api in ("dgrad", "dgrad_s2", "halo_dgrad"):
        y, bf16_out, faces = C.dgrad_exact(c), True, o.get("g")
    else:
        y, bf16_out, faces = C.wgrad_exact(c), False, o.get("x")[..., :c.creal]
    assert float(y.abs().max()) < C.LIMIT and C.worst_sum(c) < C.LIMIT
    if c.api == "dgrad_s2" and c.k == 1 and not c.acc:
        assert not y[:, 1::2].any() and not y[:, :, 1::2].any() and not y[:, :, :, 1::2].any()
    if c.api == "dgrad_s2" and c.k == 1:      # a 1^3 / stride-2 layer reaches the even-coordinate voxels only: the shares are of THOSE
        y = y[:, ::2, ::2, ::2]
    assert float((y != 0).double().mean()) >= 0.5
    if bf16_out:
        assert _frac_unrepresentable(y) >= 0.01
    if c.k > 1 and c.api not in ("fwd_occ", "wgrad_occ"):
        for d in (1, 2, 3):
            assert faces.select(d, 0).any() and faces.select(d, -1).any()
    if c.api == "bnstats" and (c.M // c.B) % 128 == 0:      # (the split-K launch emits no sums)
        s = C.bn_sums_exact(c)
        assert float(s[..., 1].max()) < C.LIMIT
        assert float(C.fwd_exact(c).float().bfloat16().double().abs().reshape(c.B, -1, 128, c.cout).sum(2).max()) < C.LIMIT
    if c.api in ("fwd_occ", "wgrad_occ"):
        occ = o.get("inocc")
        assert 0.3 < float(occ.float().mean()) < 0.9
        assert not o.get("x")[occ == 0].any()
        flags = C.row_occupancy_exact(c)
        assert tuple(flags.shape) == (c.B, *c.dout[:2]) and 0.1 < float((flags == 0).float().mean()) < 0.5      # rows are really skipped
        if c.api == "fwd_occ":
            assert not y[flags == 0].any()


@pytest.mark.parametrize("name", ["stem k5 s2", "dgrad_s2 k3 odd dims"])
def test_reference_against_int64_unfold(name):
    """the fp64 references against an independent int64 formulation: unfold + matmul for the forward and the weight gradient, a scatter of
    every (output voxel, tap) contribution for the data gradient"""
    c = next(c for c in C.ALL if c.name == name)
    o = C.operands(c)
    k, s, p = c.k, c.s, c.p
    x = o.get("x")[..., :c.creal].long()
    w = o.get("w").long()
    g = o.get("g").long()
    xp = F.pad(x, (0, 0, p, p, p, p, p, p))
    cols = xp.unfold(1, k, s).unfold(2, k, s).unfold(3, k, s)               # [B,Do,Ho,Wo,C,kd,kh,kw]
    assert tuple(cols.shape[1:4]) == c.dout
    cols = cols.reshape(c.M, c.creal * k ** 3)
    y = cols @ w.reshape(c.cout, -1).t()
    plain = dataclasses.replace(c, api="fwd", bias=False, relu=False, addend="", acc=False)
    assert torch.equal(y.double().reshape(c.B, *c.dout, c.cout), C.fwd_exact(plain))
    dw = g.reshape(c.M, c.cout).t() @ cols
    assert torch.equal(dw.double().reshape(c.cout, c.creal, k ** 3), C.wgrad_exact(dataclasses.replace(c, api="wgrad", acc=False)))
    dcols = g.reshape(c.M, c.cout) @ w.reshape(c.cout, -1)                  # [M, C * k^3]: what every output voxel sends to its window
    dxp = torch.zeros_like(xp)
    win = dxp.unfold(1, k, s).unfold(2, k, s).unfold(3, k, s)               # a view: overlapping windows, so add tap by tap
    dcols = dcols.reshape(c.B, *c.dout, c.creal, k, k, k)
    for kd in range(k):
        for kh in range(k):
            for kw in range(k):
                win[..., kd, kh, kw] += dcols[..., kd, kh, kw]
    D, H, W = c.din
    dx = dxp[:, p:p + D, p:p + H, p:p + W]
    assert torch.equal(dx.double(), C.dgrad_exact(dataclasses.replace(c, api="dgrad", acc=False)))

