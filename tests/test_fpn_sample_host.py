"""No GPU: the tables, operands and fp64 references of tests/fpn_sample_cases.py, checked on their own — the exactness preconditions of every
exact case, the tie share and tap coverage of the max-pool operands, the restated trilinear weight rule against rational arithmetic and
F.interpolate, the instantiations the table reaches, and the entry checks (null buffers: a refusal after a launch would have to touch a device)."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as N
import fpn_sample_cases as S
from dreg_nerf_amd import lib as L


# ------------------------------------------------------------------------------------------------ max-pool
def test_pool_reference_takes_the_first_maximum_in_scan_order():
    """F.max_pool3d's index against a brute-force first maximum (numpy argmax returns the first) on a tie-heavy 5x6x7 volume"""
    x = torch.from_numpy(np.random.RandomState(3).randint(-2, 3, size=(2, 5, 6, 7, 3)).astype(np.float64))
    y, tap, _ = S.pool_forward(x)
    win = S.pool_windows(x).numpy()
    assert np.array_equal(tap.numpy(), win.argmax(-1).astype(np.uint8))
    assert np.array_equal(y.numpy(), win.max(-1))


@pytest.mark.parametrize("c", S.POOL, ids=lambda c: c.id)
def test_pool_operands_tie_and_are_exact(c):
    o = S.pool_operands(c)
    x = o["x"]
    assert torch.equal(S.rounded(x, c.dt), x) and c.lo >= -3 and float(x.min()) >= -3 and float(x.max()) <= 3
    assert float(o["dy"].abs().max()) <= 8 and float(o["dx0"].abs().max()) <= 8          # dx sums at most eight of them and one more: exact in bf16
    y, tap, idx = S.pool_forward(x)
    win = S.pool_windows(x)
    assert torch.equal(tap, win.argmax(-1).to(torch.uint8)) or np.array_equal(tap.numpy(), win.numpy().argmax(-1).astype(np.uint8))
    valid = (win > float("-inf")).sum(-1)
    ties = (win == y[..., None]).sum(-1) >= 2
    if int(valid.max()) == 1:                    # a volume of one voxel: no window can tie
        assert (c.D, c.H, c.W) == (1, 1, 1)
        return
    share = float(ties[valid >= 2].double().mean())
    assert share >= 0.5, (c.name, share)
    dx = S.pool_backward(o["dy"], idx, c.D, c.H, c.W)
    assert torch.equal(S.rounded(dx + o["dx0"], c.dt), dx + o["dx0"]) and float(dx.abs().max()) <= 64


def test_pool_table_covers_taps_and_shapes():
    taps = set()
    for c in S.POOL:
        taps |= set(S.pool_forward(S.pool_operands(c)["x"])[1].reshape(-1).tolist())
    assert taps == set(range(27))
    for dt in (0, 1):
        cs = [c for c in S.POOL if c.dt == dt]
        ext = {e for c in cs for e in (c.D, c.H, c.W)}
        assert 1 in ext and 2 in ext and any(e % 2 for e in ext if e > 2) and any(e % 2 == 0 for e in ext if e > 2)
        assert any(c.C == S.G_of(dt) for c in cs) and any(c.C == 64 for c in cs) and any(c.B > 1 for c in cs)
        assert any((c.C // S.G_of(dt)) & (c.C // S.G_of(dt) - 1) for c in cs)            # CG not a power of two
        assert all(c.C % S.G_of(dt) == 0 for c in cs)
    assert {c.C for c in S.POOL if c.dt == 0} >= {8, 24, 40, 64} and {c.C for c in S.POOL if c.dt == 1} >= {4, 12, 64}


# ------------------------------------------------------------------------------------------------ fused stem
@pytest.mark.parametrize("c", S.STEM, ids=lambda c: c.id)
def test_stem_operands_keep_the_sums_exact(c):
    bn = c.bn()
    o = S.stem_operands(c)
    assert torch.equal(S.rounded(o["x"], 0), o["x"]) and torch.equal(S.rounded(o["dp"], 0), o["dp"])
    assert N.worst_partial(bn, o["x"]) < N.LIMIT
    assert c.C % 8 == 0 and not S.slabs_ragged(c.C // 8) and c.V >= 2
    assert L.load().dreg_bn_num_chunks(c.V) == -(-c.V // N.rows_per_chunk(c.V))
    # dbeta: at most 8 pooled gradients of size <= 8 per voxel, V voxels, B grids, onto |dbeta0| <= 50: an integer far below 2^24
    assert 64 * c.V * c.B + 50 < N.LIMIT
    assert float(o["dbeta0"].abs().max()) <= 50 and torch.equal(o["dbeta0"], o["dbeta0"].round())


def test_stem_table():
    assert [(c.B, c.D, c.H, c.W, c.C) for c in S.STEM[:3]] == [(2, 12, 10, 14, 64), (1, 9, 11, 7, 16), (3, 2, 2, 2, 8)]
    assert S.slabs_ragged(2056 // 8) and any(e[1] == "stem_fwd" and e[2] == 2056 for e in S.EINVAL)
    big = [c for c in S.STEM if c.C > 2048]
    assert [c.C for c in big] == [4096] and all(S.slabs_ragged(C // 8) for C in range(2056, 4096, 8))


def test_stem_restatement_matches_the_fp64_activation():
    """the fp32 selector expression stays within bn_cases' forward bound of the fp64 BatchNorm-ReLU, so it selects what the layer computes"""
    c = S.STEM[1]
    bn, o = c.bn(), S.stem_operands(c)
    f = N.forward(bn, o["x"], o["gamma"], o["beta"])
    ss = torch.stack([f["sc"], f["sh"]], -1).float()
    act, _ = S.stem_activation(o["x"].reshape(c.B, c.D, c.H, c.W, c.C), ss, True)
    tol = f["y_tol"] + 2 * N.g_(4) * (o["x"] * f["sc"][:, None]).abs() + 2 * f["sh_tol"][:, None]       # + the rounding of sc and sh to fp32
    assert bool(((act.reshape(c.B, c.V, c.C) - f["y"]).abs() <= tol).all())


# ------------------------------------------------------------------------------------------------ downsample-sum
@pytest.mark.parametrize("c", S.DOWN, ids=lambda c: c.id)
def test_downsample_reference(c):
    g = S.down_operands(c)
    out = S.down_reference(c, g)
    assert all(f in (2 * n, 2 * n - 1) for f, n in zip(c.fine, c.coarse)) and c.B == 2 and c.C % S.G_of(c.dt) == 0
    assert torch.equal(S.rounded(out, c.dt), out) and torch.equal(S.rounded(g, c.dt), g) and float(out.sum()) == float(g.sum())
    b, z, y, x = 1, c.coarse[0] - 1, c.coarse[1] - 1, c.coarse[2] - 1                    # the (possibly cropped) last parent, by hand
    want = sum(g[b, zz, yy, xx] for zz in (2 * z, 2 * z + 1) if zz < c.fine[0] for yy in (2 * y, 2 * y + 1) if yy < c.fine[1]
               for xx in (2 * x, 2 * x + 1) if xx < c.fine[2])
    assert torch.equal(out[b, z, y, x], want)
    assert S.rounded(torch.tensor([S.DOWN_SENTINEL]), 0).item() == S.DOWN_SENTINEL and float(out.abs().max()) < S.DOWN_SENTINEL
    n = c.B * c.coarse[0] * c.coarse[1] * c.coarse[2]
    for kind in S.ROW_LISTS:
        rows = S.down_rows(c, kind)
        assert rows.dtype == np.int32 and np.all(np.diff(rows) > 0) and (len(rows) == 0 or (rows[0] >= 0 and rows[-1] < n))
    assert len(S.down_rows(c, "full")) == n and len(S.down_rows(c, "one")) == 1 and len(S.down_rows(c, "empty")) == 0


def test_downsample_table_covers_both_crops_on_every_axis():
    for ax in range(3):
        assert {c.fine[ax] - 2 * c.coarse[ax] for c in S.DOWN} == {0, -1}
    assert {(c.C, c.dt) for c in S.DOWN} == {(8, 0), (24, 0), (4, 1), (12, 1)}


# ------------------------------------------------------------------------------------------------ trilinear: the weight rule
ALL_PAIRS = sorted(set(S.EXACT_PAIRS + S.GENERAL_PAIRS + S.SWEEP_BIG + tuple((no, ni) for _, no, ni in S.SWEEP)))


def test_axis_weights_against_rational_align_corners():
    for n_out, n_in in ALL_PAIRS:
        i0, i1, t, _ = S.tri_axis(n_out, n_in)
        for i in range(n_out):
            pos = Fraction(i * (n_in - 1), n_out - 1) if n_out > 1 else Fraction(0)
            got = np.zeros(n_in)
            got[i0[i]] += 1.0 - float(t[i])
            got[i1[i]] += float(t[i])
            lo = min(int(pos), n_in - 1)
            want = np.zeros(n_in)
            want[lo] += float(1 - (pos - lo))
            if pos != lo:
                want[lo + 1] += float(pos - lo)
            assert np.abs(got - want).max() <= S.axis_bound(n_in), (n_out, n_in, i)


def test_exact_pairs_have_exact_coordinates():
    for n_out, n_in in S.EXACT_PAIRS:
        _, _, t, f = S.tri_axis(n_out, n_in)
        f64 = np.arange(n_out, dtype=np.float64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        assert np.array_equal(f.astype(np.float64), f64), (n_out, n_in)
        assert np.array_equal(t * 4, np.round(t * 4))                  # every per-axis weight a multiple of 1/4: corner weights of 1/64
    assert {p for c in S.TRI_EXACT for p in (c.z, c.x, c.y)} == set(S.EXACT_PAIRS)
    assert {p for c in S.TRI_GENERAL for p in (c.z, c.x, c.y)} == set(S.GENERAL_PAIRS)
    assert all(len({c.z, c.x, c.y}) == 3 for c in S.TRI) and any(1 in c.fine and 1 in c.coarse for c in S.TRI_EXACT)


def test_forward_reference_is_interpolate_gathered_at_idx():
    """all three extents differ, fine and coarse: pins (z, x, y) <-> (d, h, w) and the (x Yr + y) Zr + z order independently of the restatement"""
    for c in (S.TriCase("anchor", (10, 5), (12, 6), (14, 7), 8, False), S.TriCase("anchor", (7, 13), (9, 3), (13, 4), 8, True)):
        o = S.tri_operands(c)
        geom, p1 = o["geom"], o["p1"][1]
        out, mag = S.tri_forward(geom, p1)
        Zr, Xr, Yr = c.fine
        up = F.interpolate(p1.permute(0, 4, 1, 2, 3), size=(Zr, Xr, Yr), mode="trilinear", align_corners=True)     # [B, C, Zr, Xr, Yr]
        idx = torch.from_numpy(geom.idx)
        z, y, x = idx % Zr, (idx // Zr) % Yr, idx // (Zr * Yr)
        want = up[torch.from_numpy(geom.pt_batch).long(), :, z, x, y]
        vsum = torch.zeros_like(out)
        flat = p1.reshape(-1, c.C)
        for k in range(8):
            vsum += flat[torch.from_numpy(geom.row[:, k])].abs()
        bound = vsum * sum(S.axis_bound(n) for n in c.coarse) + 1e-14 * vsum
        assert bool(((out - want).abs() <= bound).all()), c.name
        assert float((out - want).abs().max()) < 1e-5 and float(out.abs().max()) > 0.5
        assert np.abs(geom.w.astype(np.float64).sum(1) - 1).max() <= 8 * S.U


# ------------------------------------------------------------------------------------------------ trilinear: the cases
@pytest.mark.parametrize("c", S.TRI, ids=lambda c: c.id)
def test_tri_case_geometry(c):
    o = S.tri_operands(c)
    geom = o["geom"]
    Zr, Xr, Yr = c.fine
    Vf = Zr * Xr * Yr
    key = geom.pt_batch.astype(np.int64) * Vf + geom.idx
    assert len(np.unique(key)) == len(key) and geom.idx.min() >= 0 and geom.idx.max() < Vf          # fine_map holds one point per voxel
    present = set(geom.pt_batch.tolist())
    assert 1 not in present and present == set(range(c.B)) - {1}                                     # one grid without a point
    for b in present:
        assert Vf - 1 in set(geom.idx[geom.pt_batch == b].tolist())                                 # the clamped last voxel of every axis
    assert np.all(np.diff(geom.rows1) > 0) and geom.rows1.max() < geom.nrows
    assert np.array_equal(geom.map1[geom.rows1], np.arange(len(geom.rows1))) and (geom.map1 >= 0).sum() == len(geom.rows1)
    assert set(geom.row[geom.w != 0].tolist()) <= set(geom.rows1.tolist()) and len(geom.rows1) < geom.nrows
    if c.seg:
        assert c.B == 4 and len(o["plans"]) == 2
        start = 0
        for p in o["plans"]:
            assert p.point_start == start and set((geom.pt_batch[start:start + p.n] // 2).tolist()) == {len([q for q in o["plans"] if q.point_start < start])}
            assert sorted(p.order.tolist()) == list(range(p.n)) and int(p.starts[-1]) == p.n and np.all(np.diff(p.starts.astype(np.int64)) >= 1)
            sizes = np.diff(p.starts.astype(np.int64))
            assert set(sizes.tolist()) <= ({1, 2, 4, 8} if c.exact else set(range(1, 9))) and len(set(sizes.tolist())) >= 3
            for s in range(p.nseg):
                mem = p.order[p.starts[s]:p.starts[s + 1]]
                assert np.all(p.inv_seg[mem] == s) and np.all(p.inv_cnt[mem] == np.float32(1) / np.float32(len(mem)))
            start += p.n
        assert start == len(geom.idx) and o["g1"].shape[0] == sum(p.nseg for p in o["plans"])
    else:
        assert c.B == 3


@pytest.mark.parametrize("c", S.TRI_EXACT, ids=lambda c: c.id)
def test_preconditions_of_the_exact_regime(c):
    o = S.tri_operands(c)
    geom = o["geom"]
    assert np.array_equal(geom.w * 64, np.round(geom.w * 64)) and not geom.merged.any()
    for key in ("dfeat", "g1"):
        if key in o:
            assert torch.equal(o[key], o[key].round()) and float(o[key].abs().max()) <= 8
    p1 = o["p1"][0]
    assert torch.equal(p1, p1.round()) and float(p1.abs().max()) <= 8 and torch.equal(o["p1"][1], p1)
    out, mag = S.tri_forward(geom, p1)
    assert torch.equal(out * 64, (out * 64).round()) and float(mag.max()) * 64 < S.LIMIT
    if c.label == "E1":                                                                              # some bf16 stores of the forward really round
        assert float((S.rounded(out, 0) != out).double().mean()) > 0.001
    dp, mag_b, K, mag_m = S.tri_backward(geom, o["dfeat"])
    assert torch.equal(dp * 64, (dp * 64).round()) and float(mag_b.max()) * 64 < S.LIMIT and float(mag_m.max()) == 0
    if c.label == "E1":                                                                              # and many of the backward; a voxel with > 64 terms
        assert float((S.rounded(dp, 0) != dp).double().mean()) > 0.05 and float(K.max()) > 64
    if c.seg:
        for p in o["plans"]:
            mean, m, cnt = S.tri_segment_mean(p, out, mag)
            assert torch.equal(mean * 512, (mean * 512).round()) and float(m.max()) * 64 < S.LIMIT
        df = S.seg_dfeat(o["plans"], o["g1"], len(geom.idx))
        dps, mags, _, _ = S.tri_backward(geom, df)
        assert torch.equal(df * 8, (df * 8).round()) and torch.equal(dps * 512, (dps * 512).round()) and float(mags.max()) * 512 < S.LIMIT


def test_general_regime_operands():
    merged = 0
    for c in S.TRI_GENERAL:
        o = S.tri_operands(c)
        assert torch.equal(S.rounded(o["p1"][0], 0), o["p1"][0]) and torch.equal(o["p1"][1].float().double(), o["p1"][1])
        assert not torch.equal(o["p1"][0], o["p1"][1]) and torch.equal(o["dfeat"].float().double(), o["dfeat"])
        merged += int(o["geom"].merged.sum())
        _, _, K, _ = S.tri_backward(o["geom"], o["dfeat"][:, :1])
        assert float(K.max()) >= 8
    print(f"points with a clamped axis and t != 0 over the general cases: {merged}")


def test_table_reaches_every_instantiation():
    for group in (S.TRI_EXACT, S.TRI_GENERAL):
        got = set()
        for c in group:
            assert c.insts <= S.INSTANTIATIONS and c.insts
            got |= c.insts
        assert got == S.INSTANTIATIONS, S.INSTANTIATIONS - got
    assert len(S.INSTANTIATIONS) == 5 + 3 + 16
    assert {c.C for c in S.TRI_EXACT} >= {8, 24, 64, 128, 192, 256}


def test_sweep_table():
    assert {(no, ni) for ax, no, ni in S.SWEEP if ax == 0} >= {(no, ni) for ni in range(1, 11) for no in range(1, 21)}
    for ax in range(3):
        assert {(no, ni) for a, no, ni in S.SWEEP if a == ax} >= set(S.SWEEP_BIG)
    c = S.sweep_case(1, 200, 3)
    geom, g = S.sweep_operands(c)
    assert c.fine == (1, 200, 1) and c.coarse == (1, 3, 1) and len(geom.idx) == 200 and len(geom.rows1) == 3
    _, _, K, _ = S.tri_backward(geom, g)
    assert float(K.max()) > 64 * 2                                                                   # several rounds of the 64-lane candidate loop
    assert sum(len(S.sweep_operands(S.sweep_case(*s))[0].idx) for s in S.SWEEP) < 10000


# ------------------------------------------------------------------------------------------------ entry checks
@pytest.mark.parametrize("what,entry,C,dt,extra", S.EINVAL, ids=[f"{e[1]}_{e[0]}".replace(" ", "_").replace(",", "").replace("%", "mod").replace(">", "gt") for e in S.EINVAL])
def test_refused_calls_return_einval_before_any_launch(what, entry, C, dt, extra):
    assert S.refused_call(L.load(), entry, C, dt, extra) == -1, (what, entry)


def test_einval_table_covers_the_entries():
    entries = {e[1] for e in S.EINVAL}
    assert entries >= {"maxpool_fwd", "maxpool_bwd_acc", "maxpool_bwd", "downsample_sum", "gather_fwd", "bwd_gather", "bwd_gather_rows_only",
                       "bwd_gather_seg", "segment_mean", "stem_fwd", "stem_bwd"}
    for entry in ("maxpool_fwd", "maxpool_bwd_acc", "downsample_sum", "gather_fwd"):
        assert {e[3] for e in S.EINVAL if e[1] == entry} == {0, 1}
    for entry in ("bwd_gather", "bwd_gather_rows_only", "bwd_gather_seg"):
        assert {e[2] for e in S.EINVAL if e[1] == entry} >= {96, 320}


def test_no_layer_hands_these_entries_a_ragged_channel_count():
    """the channel widths that reach the pooling / gather entries: the ResNet stem and the FPN head (dreg_nerf_amd/regtr.py)"""
    from dreg_nerf_amd import params
    sd = params.synth_state_dict(0)
    widths = {int(v.shape[0]) for k, v in sd.items() if k.startswith("fpn3d.") and k.endswith(".weight") and v.dim() == 5}
    assert widths and all(w % 8 == 0 for w in widths), widths
