"""GPU: the scene density field (csrc/scene_field.hip, dreg_nerf_amd/scene_field.py; rule: DESIGN.md §3k; restatement: tests/scene_field_restatement.py)
on the four generated 32^3 blocks, centroids and poses of tests/test_hip_render_scene.py.

* K = 2 with [(src, P), (tgt, None)] IS dreg_pair_density, bit for bit, in all five outputs, in the points form and the lattice form; K = 1 is the
  block's masked query; with every grid empty but two / but one / all empty, K = 3 and 4 are the pair's outputs / the block's masked query / zeros.
* The parts are the blocks' own dense queries bit for bit, masked by a torch statement of the coverage rule; the weights are 0 / 1 / fl(1 - w_lo)
  where the rule says so; the blend is exact given its parts.
* The weights against the fp64 restatement where two or more blocks cover.  With y_j = p/2 ln(delta_b / delta_j): |d omega / d y_j| =
  omega^2 e^(y_j) <= omega (1 - omega) <= 1/4 and the sum over j of those derivatives is omega (1 - omega) too, so |d omega| <= max_j |dy_j| / 4;
  |dy| <= |y| 2^-21 + 2^-20 (§3i: native exp2 / log2 within 2 ulp and the roundings of their argument scalings) at |y| <= 3.8 (asserted), plus
  the K - 1 additions and the division at 2^-24 each: 6.9e-7 + K 6.0e-8, and the bound is 8 times that (§3i's margin over its own derivation).
  The test prints the largest |d omega| it saw and max |y| (DESIGN.md §3k records them).
* The same block K times under no pose: omega = 1/K, the field is the masked block.
* Lattice form == points form; permutations permute; two runs give identical bytes.
* scene_mesh at resolution 24; with K = 2 it is pair_mesh bit for bit.  Every C guard with sentinels; the Python guards;
  eval_nerf_regtr.py --scene_mesh_field on a three-block split on disk."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mc_restatement as M
import scene_field_restatement as SF
import test_hip_pair_field as TPF
import test_hip_render_pair as TP
import test_hip_render_scene as TS
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import mesh, ngp
from dreg_nerf_amd import pair_field as P
from dreg_nerf_amd import render as R
from dreg_nerf_amd import scene_field as S

pytestmark = pytest.mark.gpu
DEV, AABB = TP.DEV, TP.AABB
CENTERS, POSES = TS.CENTERS, TS.POSES
_same, _bits, _nodes, _covered_torch, _to_block_torch = TPF._same, TPF._bits, TPF._nodes, TPF._covered_torch, TPF._to_source_torch
Y_MAX = 3.8                                   # the premise of the weights' bound: max |p/2 ln(delta_b / delta_b')| over the shared test points


def _bound(K):
    return 8.0 * (0.25 * (Y_MAX * 2.0 ** -21 + 2.0 ** -20) + K * 2.0 ** -24)


def _empty():
    return ngp.OccupancyGrid(AABB, 32)


def _field(four, K, grids=None, poses=None, power=4.0):
    grids = [four[b][1] for b in range(K)] if grids is None else grids
    poses = TS._poses(K) if poses is None else poses
    return S.SceneField([(four[b][0], grids[b], CENTERS[b], poses[b]) for b in range(K)], power=power)


@pytest.fixture(scope="module")
def four():
    return [TP._block(seed, shell=shell) for seed, shell in TS.SHELLS]


@pytest.fixture(scope="module")
def x():
    """8,192 points of the scene frame, uniform in [-1.2, 1.2]^3."""
    return ((torch.rand(8192, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1) * 1.2).contiguous().to(DEV)


def _reference(four, x, K):
    """The points in every block's frame, their coverages from the torch statement of the rule, the blocks' own queries and the kernel's parts for
    the K-block scene of tests/test_hip_render_scene.py — computed once and left unchanged.  The condition is asserted first: every coverage count
    0 .. K holds at least 200 of the points (checked on the CPU coverage rule when the numbers were fixed: 5384 / 674 / 555 / 1579 at K = 3 and
    5003 / 629 / 523 / 551 / 1486 at K = 4)."""
    poses = TS._poses(K)
    xb = [x if p is None else _to_block_torch(x, p) for p in poses]
    m = torch.stack([_covered_torch(four[b][1], xb[b]) for b in range(K)], dim=1)
    cnt = m.sum(dim=1)
    counts = [int((cnt == c).sum()) for c in range(K + 1)]
    print(f"K = {K}: points per coverage count {counts}")
    assert min(counts) >= 200, counts
    sf = _field(four, K)
    sigma, wb, sb = sf.query(x, parts=True)
    own = torch.stack([four[b][0].query_raw(xb[b].contiguous())[0] for b in range(K)], dim=1)
    return dict(K=K, poses=poses, xb=xb, m=m, cnt=cnt, sf=sf, sigma=sigma, wb=wb, sb=sb, own=own)


@pytest.fixture(scope="module")
def refs(four, x):
    return {K: _reference(four, x, K) for K in (3, 4)}


@pytest.fixture(scope="module")
def pf(four):
    return P.PairField(four[0][0], four[0][1], four[1][0], four[1][1], POSES[0], CENTERS[0], CENTERS[1])


# ------------------------------------------------------------------------------------------------------- exactness against the existing kernels
def test_two_blocks_are_the_pair_density_bit_for_bit_in_both_forms(four, x, pf):
    sf = _field(four, 2, poses=[POSES[0], None])
    want = pf.query(x, parts=True)                                            # sigma, w_src, w_tgt, sigma_src, sigma_tgt
    sigma, wb, sb = sf.query(x, parts=True)
    both = (want[1] > 0) & (want[2] > 0)
    assert int(both.sum()) > 1000 and float(want[0].max()) > 1.0
    assert _same(sigma, want[0]) and _same(wb[:, 0], want[1]) and _same(wb[:, 1], want[2]) and _same(sb[:, 0], want[3]) and _same(sb[:, 1], want[4])
    assert sf.lattice(16) == pf.lattice(16) and sf.lattice(24) == pf.lattice(24)
    for power in (1.5,):                                                      # another exponent of the overlap weight
        a = _field(four, 2, poses=[POSES[0], None], power=power).query(x, parts=True)
        b = P.PairField(four[0][0], four[0][1], four[1][0], four[1][1], POSES[0], CENTERS[0], CENTERS[1], power=power).query(x, parts=True)
        assert _same(a[0], b[0]) and _same(a[1][:, 0], b[1]) and _same(a[1][:, 1], b[2]) and not _same(a[0], sigma)
    origin, spacing, dims = pf.lattice(16)
    assert dims == (19, 19, 16)
    n = dims[0] * dims[1] * dims[2]
    want = pf._run(None, n, origin, spacing, dims, True)
    sigma, wb, sb = sf._run(None, n, origin, spacing, dims, True)
    assert int((want[0] > 0.7).sum()) > 50
    assert _same(sigma, want[0]) and _same(wb[:, 0], want[1]) and _same(wb[:, 1], want[2]) and _same(sb[:, 0], want[3]) and _same(sb[:, 1], want[4])
    assert _same(sf.sample_lattice(origin, spacing, dims), pf.sample_lattice(origin, spacing, dims))


def test_one_block_without_a_pose_is_its_masked_query(four, x):
    sf = _field(four, 1, poses=[None])
    sigma, wb, sb = sf.query(x, parts=True)
    m = _covered_torch(four[0][1], x)
    own = four[0][0].query_raw(x)[0]
    assert int(m.sum()) > 1000 and int((~m).sum()) > 1000
    assert _same(sigma, own * m) and _same(sb[:, 0], own * m) and _same(wb[:, 0], m.float()) and wb.shape == (8192, 1)
    assert _same(sf.query(x), sigma)
    # through a pose: the block's masked query at the moved points
    xs = _to_block_torch(x, POSES[0])
    ms = _covered_torch(four[0][1], xs)
    assert _same(_field(four, 1, poses=[POSES[0]]).query(x), four[0][0].query_raw(xs)[0] * ms)


@pytest.mark.parametrize("K,i", [(3, 0), (3, 1), (4, 0), (4, 1), (4, 2)])
def test_all_grids_empty_but_two_are_the_pairs_outputs(four, x, K, i):
    last = K - 1
    poses = list(POSES[:last]) + [None]
    grids = [four[b][1] if b in (i, last) else _empty() for b in range(K)]
    sigma, wb, sb = _field(four, K, grids=grids, poses=poses).query(x, parts=True)
    want = P.PairField(four[i][0], four[i][1], four[last][0], four[last][1], POSES[i], CENTERS[i], CENTERS[last]).query(x, parts=True)
    assert int(((want[1] > 0) & (want[2] > 0)).sum()) > 1000
    assert _same(sigma, want[0]) and _same(wb[:, i], want[1]) and _same(wb[:, last], want[2]) and _same(sb[:, i], want[3]) and _same(sb[:, last], want[4])
    others = [b for b in range(K) if b not in (i, last)]
    assert not wb[:, others].any() and not sb[:, others].any()


@pytest.mark.parametrize("K", [3, 4])
def test_all_grids_empty_but_one_is_that_blocks_masked_query_and_all_empty_is_zero(four, x, refs, K):
    r = refs[K]
    for i in range(K):
        grids = [four[b][1] if b == i else _empty() for b in range(K)]
        sigma, wb, sb = _field(four, K, grids=grids).query(x, parts=True)
        want = r["own"][:, i] * r["m"][:, i]
        assert float(want.max()) > 1.0 and _same(sigma, want) and _same(sb[:, i], want) and _same(wb[:, i], r["m"][:, i].float()), i
        others = [b for b in range(K) if b != i]
        assert not wb[:, others].any() and not sb[:, others].any(), i
    sf = _field(four, K, grids=[_empty() for _ in range(K)])
    sigma, wb, sb = sf.query(x, parts=True)
    assert _same(sigma, torch.zeros_like(sigma)) and _same(wb, torch.zeros_like(wb)) and _same(sb, torch.zeros_like(sb))
    origin, spacing, dims = sf.lattice(16)
    values = sf.sample_lattice(origin, spacing, dims)
    assert _same(values, torch.zeros_like(values))


# ------------------------------------------------------------------------------------------------------- parts, weights, blend
@pytest.mark.parametrize("K", [3, 4])
def test_parts_are_the_blocks_own_queries_and_the_weights_follow_the_rule(refs, K):
    r = refs[K]
    m, cnt, wb, sb = r["m"], r["cnt"], r["wb"], r["sb"]
    for b in range(K):
        assert _same(sb[:, b], r["own"][:, b] * m[:, b]), b
        assert float(sb[:, b][m[:, b]].min()) > 0
        assert torch.equal(r["sf"].covered(b, r["xb"][b]), m[:, b])
    assert (wb[~m] == 0).all()
    assert (wb[m & (cnt == 1)[:, None]] == 1).all()
    shared = wb[m & (cnt >= 2)[:, None]]
    assert ((shared > 0) & (shared < 1)).all()
    # exactly two blocks cover: the higher index carries fl(1 - omega_lo)
    two = cnt == 2
    idx = torch.arange(K, device=DEV)[None, :].expand_as(m)
    lo = torch.where(m, idx, torch.full_like(idx, K)).min(dim=1).values[two]
    hi = torch.where(m, idx, torch.full_like(idx, -1)).max(dim=1).values[two]
    w_lo, w_hi = wb[two].gather(1, lo[:, None])[:, 0], wb[two].gather(1, hi[:, None])[:, 0]
    assert int(two.sum()) >= 200 and _same(w_hi, 1.0 - w_lo)
    tot = wb.double().sum(dim=1)
    assert float((tot[cnt > 0] - 1.0).abs().max()) <= K * 2.0 ** -23 and (tot[cnt == 0] == 0).all()
    one = cnt == 1
    assert _same(r["sigma"][one], (r["own"] * m)[one].sum(dim=1)) and (r["sigma"][cnt == 0] == 0).all()


@pytest.mark.parametrize("K", [3, 4])
def test_points_to_block_is_the_kernels_expression(refs, x, K):
    r = refs[K]
    for b in range(K):
        got = r["sf"].points_to_block(b, x)
        assert _same(got, r["xb"][b]), b
        if r["poses"][b] is None:
            assert got is x


@pytest.mark.parametrize("K", [3, 4])
def test_the_blend_is_exact_given_its_parts(refs, K):
    r = refs[K]
    p = [r["wb"][:, b] * r["sb"][:, b] for b in range(K)]
    want = p[0] + p[1]
    for b in range(2, K):
        want = want + p[b]
    assert _same(r["sigma"], want)
    full = r["cnt"] == K
    for b in range(K):
        assert not _same(r["sigma"][full], r["sb"][:, b][full])


@pytest.mark.parametrize("K", [3, 4])
def test_weights_against_fp64(refs, K):
    r = refs[K]
    m = r["m"].cpu().numpy()
    xs = [v.cpu().numpy() for v in r["xb"]]
    delta = SF.deltas(xs, [c.numpy() for c in CENTERS[:K]])
    shared = m.sum(axis=1) >= 2
    y = SF.log_ratios(m, delta, 4.0)[shared]
    assert y.max() <= Y_MAX, y.max()                                          # the premise of the bound's derivation
    want = SF.weights(m, delta, 4.0)[shared]
    got = r["wb"].cpu().numpy().astype(np.float64)[shared]
    err = float(np.abs(got - want).max())
    general = m.sum(axis=1)[shared] >= 3
    print(f"scene field weights, K = {K}: {int(shared.sum())} shared points ({int(general.sum())} under three or more blocks), max |y| {y.max():.4f}, "
          f"max |d omega| {err:.3e} (derived {_bound(K) / 8:.2e}, bound {_bound(K):.2e})")
    assert int(general.sum()) >= 200 and err <= _bound(K)
    cov = want[m[shared]]
    assert cov.min() < 0.1 and cov.max() > 0.9                                # the weights are exercised over their range


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_the_same_block_k_times_under_no_pose_shares_equally(four, x, K):
    f, occ = four[1][0], four[1][1]
    sf = S.SceneField([(f, occ, CENTERS[1], None)] * K)
    sigma, wb, sb = sf.query(x, parts=True)
    m = _covered_torch(occ, x)
    own = f.query_raw(x)[0] * m
    assert int(m.sum()) > 1000 and (wb[~m] == 0).all()
    err = float((wb[m].double() - 1.0 / K).abs().max())
    assert err <= _bound(K), err
    if K <= 2:
        assert (wb[m] == 1.0 / K).all()
    for b in range(K):
        assert _same(sb[:, b], own)
    rel = float(((sigma.double() - own.double()).abs() / own.double().clamp(min=1e-30))[m].max())
    print(f"same block {K} times: max |omega - 1/K| {err:.3e}, max relative |sigma - m sigma_b| {rel:.3e}")
    assert rel <= _bound(K) and (sigma[~m] == 0).all()


# ------------------------------------------------------------------------------------------------------- lattice form, order, repeatability
@pytest.mark.parametrize("lattice", ["19x19x16", "27x27x22", "nx_65"])
def test_lattice_form_is_the_points_form_of_its_nodes(refs, lattice):
    sf = refs[3]["sf"]
    if lattice == "nx_65":
        origin, spacing, dims = [-1.3, -0.4, -0.3], [float(np.float32(0.04)), float(np.float32(0.11)), float(np.float32(0.13))], (65, 7, 5)      # the x walk straddles a wave
    else:
        origin, spacing, dims = P.pair_lattice(AABB, AABB, POSES[0], {"19x19x16": 16, "27x27x22": 24}[lattice])
        assert "x".join(str(d) for d in dims) == lattice
    origin = [float(np.float32(v)) for v in origin]
    got = sf.sample_lattice(origin, spacing, dims)
    want = sf.query(_nodes(origin, spacing, dims))
    assert got.shape == (dims[2], dims[1], dims[0]) and _same(got.reshape(-1), want)
    assert int((got > 0.7).sum()) > 50 and int((got == 0).sum()) > 50


@pytest.mark.parametrize("K", [3, 4])
def test_a_permutation_permutes_and_two_runs_agree(refs, x, K):
    r = refs[K]
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    again = r["sf"].query(x, parts=True)
    moved = r["sf"].query(x[perm].contiguous(), parts=True)
    for k, name in enumerate(("sigma", "wb", "sb")):
        assert _same(again[k], r[name]), name
        assert _same(moved[k], r[name][perm]), name
    assert _same(r["sf"].query(x[:100].reshape(10, 10, 3)), r["sigma"][:100].reshape(10, 10))
    assert r["sf"].query(x[:100].reshape(10, 10, 3), parts=True)[1].shape == (10, 10, K)
    origin, spacing, dims = r["sf"].lattice(16)
    assert _same(r["sf"].sample_lattice(origin, spacing, dims), r["sf"].sample_lattice(origin, spacing, dims))


# ------------------------------------------------------------------------------------------------------- the mesh of the scene
def test_scene_mesh_is_one_closed_surface(refs):
    sf = refs[3]["sf"]
    origin, spacing, dims = sf.lattice(24)
    values = sf.sample_lattice(origin, spacing, dims)
    shell = torch.ones_like(values, dtype=torch.bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert (values[shell] == 0).all() and int((values[~shell] > 0.7).sum()) > 100
    m = S.scene_mesh(sf, 24, level=0.7)
    verts, faces = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    assert m["level"] == 0.7 and m["dims"] == dims and len(verts) > 500 and len(faces) > 500
    v, f = mesh.marching_cubes(values, 0.7, origin, spacing)
    assert _same(m["verts"], v) and torch.equal(m["faces"], f)
    assert M.is_closed(faces) and M.repeated_index_faces(faces) == 0 and not M.unmatched_edges(faces)
    assert M.signed_volume(verts, faces) > 0
    area, vol = mesh.mesh_area_volume(m["verts"], m["faces"])
    assert vol == pytest.approx(M.signed_volume(verts, faces), rel=1e-9) and area > 0
    n2 = (m["normals"].double() ** 2).sum(dim=1)
    assert (((n2 - 1).abs() <= 1e-5) | (n2 == 0)).all() and int((n2 > 0).sum()) > len(verts) // 2
    col, share = m["colors"], m["share"]
    assert col.shape == m["verts"].shape and float(col.min()) >= 0 and float(col.max()) <= 1
    assert share.shape == (len(verts), 3) and float(share.min()) >= 0 and float(share.max()) <= 1
    tot = share.double().sum(dim=1)
    assert (((tot - 1).abs() <= 3 * 2.0 ** -23) | ((tot == 0) & (share == 0).all(dim=1))).all()
    three = int((share > 0).all(dim=1).sum())
    print(f"scene_mesh resolution 24, K = 3: V {len(verts)} F {len(faces)} area {area:.3f} volume {vol:.3f}; vertices shared by three blocks {three}")
    assert three > 0
    bare = S.scene_mesh(sf, 24, level=0.7, normals=False, colors=False)
    assert bare["normals"] is None and bare["colors"] is None and torch.equal(bare["faces"], m["faces"]) and _same(bare["share"], share)
    assert S.scene_mesh(sf, 24)["level"] == mesh.DENSITY_THRE


def test_scene_mesh_of_two_blocks_is_pair_mesh_bit_for_bit(four, pf):
    sf = _field(four, 2, poses=[POSES[0], None])
    want = P.pair_mesh(pf, 24, level=0.7)
    got = S.scene_mesh(sf, 24, level=0.7)
    assert want["verts"].shape[0] > 500 and got["dims"] == want["dims"] == (27, 27, 22) and got["origin"] == want["origin"] and got["spacing"] == want["spacing"]
    assert _same(got["verts"], want["verts"]) and torch.equal(got["faces"], want["faces"])
    assert _same(got["colors"], want["colors"]) and _same(got["normals"], want["normals"]) and _same(got["share"][:, 0], want["weight_src"])
    assert int(((want["weight_src"] > 0) & (want["weight_src"] < 1)).sum()) > 50


# ------------------------------------------------------------------------------------------------------- guards
def test_every_c_guard_returns_einval_without_a_launch(refs, x, pf):
    lib = L.load()
    sf = refs[3]["sf"]
    keep = []
    arr = sf._block_array(keep)
    SENT = -77.0
    n = 256
    xs = x[:n].contiguous()
    sigma, wb, sb = torch.full((n,), SENT, device=DEV), torch.full((n, 3), SENT, device=DEV), torch.full((n, 3), SENT, device=DEV)
    outs = [sigma, wb, sb]
    org, spc = (ctypes.c_float * 3)(-1.0, -1.0, -1.0), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    s = L.stream()
    blocks_p = ctypes.cast(arr, ctypes.c_void_p)

    def call(x_=L.ptr(xs), n_=n, o=None, sp=None, dims=(0, 0, 0), K=3, blocks=blocks_p, power=4.0, sigma_=L.ptr(sigma), rest=(L.ptr(wb), L.ptr(sb))):
        return lib.dreg_scene_density(x_, n_, o, sp, *dims, K, blocks, power, sigma_, *rest, s)

    def with_field(k, name, v, **kw):
        saved = getattr(arr[k], name)
        setattr(arr[k], name, v)
        try:
            return call(**kw)
        finally:
            setattr(arr[k], name, saved)
    lat = lambda **kw: call(**{**dict(x_=None, n_=0, o=org, sp=spc, dims=(4, 4, 4)), **kw})
    bad = [call(K=0), call(K=5), call(K=-1), call(blocks=None), lat(K=0), lat(K=5), lat(blocks=None)]
    bad += [call(x_=None), call(sigma_=None), call(n_=-1), call(n_=-1, x_=None)]
    pointers = [nm for nm, _ in L.FieldBlock._fields_ if nm not in ("rx", "ry", "rz", "pose")]
    assert len(pointers) == 12
    for k in range(3):
        bad += [with_field(k, nm, None) for nm in pointers]                                            # every pointer of the block but the pose
        bad += [with_field(k, nm, v) for nm, v in (("rx", 0), ("ry", -1), ("rz", 0))]                  # an occupancy-grid dimension <= 0
    bad += [call(power=p) for p in (0.0, -1.0, float("nan"), float("inf"), -float("inf"))]
    bad += [lat(dims=d) for d in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -3, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025), (1024, 1024, 257))]
    bad += [lat(o=None), lat(sp=None), lat(x_=L.ptr(xs)), lat(sigma_=None), lat(n_=-1), lat(power=0.0), with_field(0, "binary", None, **dict(x_=None, n_=0, o=org, sp=spc, dims=(4, 4, 4))),
            with_field(2, "rz", 0, **dict(x_=None, n_=0, o=org, sp=spc, dims=(4, 4, 4)))]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs), "a refused call wrote to the device"
    # a null pose is no error: the block takes the points as they are (block 2 of this scene has none already)
    assert arr[2].pose is None and arr[0].pose is not None
    # n == 0: OK, nothing launched, whatever the pointers
    assert call(n_=0) == 0 and call(n_=0, x_=None, sigma_=None, rest=(None, None)) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs)
    assert sf.query(torch.empty(0, 3, device=DEV)).shape == (0,)
    empty_parts = sf.query(torch.empty(0, 3, device=DEV), parts=True)
    assert empty_parts[1].shape == (0, 3) and empty_parts[2].shape == (0, 3)
    # the optional outputs are optional; a good call writes what the wrapper returns
    assert call(rest=(None, None)) == 0
    torch.cuda.synchronize()
    assert _same(sigma, refs[3]["sigma"][:n]) and bool((wb == SENT).all()) and bool((sb == SENT).all())
    assert call(rest=(L.ptr(wb), None)) == 0
    torch.cuda.synchronize()
    assert _same(wb, refs[3]["wb"][:n]) and bool((sb == SENT).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert _same(sigma, refs[3]["sigma"][:n]) and _same(wb, refs[3]["wb"][:n]) and _same(sb, refs[3]["sb"][:n])
    small = torch.full((64,), SENT, device=DEV)
    assert lat(sigma_=L.ptr(small), rest=(None, None)) == 0
    torch.cuda.synchronize()
    assert _same(small.view(4, 4, 4), sf.sample_lattice([-1.0] * 3, [0.25] * 3, (4, 4, 4)))


def test_python_guards(four, refs):
    f = [b[0] for b in four]
    g = [b[1] for b in four]
    mk = lambda fields, grids, poses, **kw: S.SceneField([(fields[b], grids[b], CENTERS[b % 4], poses[b]) for b in range(len(fields))], **kw)
    f[1].unbounded = True
    try:
        with pytest.raises(NotImplementedError):
            mk(f[:3], g[:3], TS._poses(3))
    finally:
        f[1].unbounded = False
    contracted = R.BlockGrid(AABB, g[1].binary.to(DEV).view(torch.uint8), contraction_type=ngp.ContractionType.UN_BOUNDED_SPHERE)
    with pytest.raises(NotImplementedError):
        mk(f[:3], [g[0], contracted, g[2]], TS._poses(3))
    cpu_field = ngp.NGPradianceField(AABB).eval()
    with pytest.raises(ValueError):
        mk([cpu_field, f[1], f[2]], g[:3], TS._poses(3))                      # the first block on the host
    with pytest.raises(ValueError):
        mk([f[0], cpu_field, f[2]], g[:3], TS._poses(3))                      # mixed devices
    for power in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mk(f[:3], g[:3], TS._poses(3), power=power)
    with pytest.raises(ValueError):
        S.SceneField([])
    with pytest.raises(ValueError):
        mk(f + f[:1], g + g[:1], list(POSES) + [None])
    with pytest.raises(ValueError):
        mk(f[:2], g[:2], [torch.eye(3), None])
    sf = refs[3]["sf"]
    with pytest.raises(ValueError):
        sf.query(torch.zeros(4, 3))
    for dims in ((1, 4, 4), (4, 4, 1025), (1024, 1024, 257)):
        with pytest.raises(ValueError):
            sf.sample_lattice([0.0] * 3, [0.1] * 3, dims)
    blk = R.BlockGrid(AABB, g[0].binary.to(DEV).view(torch.uint8))
    p = torch.zeros(1, 3, device=DEV) + 0.7
    assert _same(mk(f[:3], [blk, g[1], g[2]], [q if q is None else q[:3] for q in TS._poses(3)]).query(p), sf.query(p))


# ------------------------------------------------------------------------------------------------------- the evaluator's flag on disk
def test_evaluator_scene_mesh_field_on_a_three_block_tree(four, tmp_path, monkeypatch, capsys):
    """eval_nerf_regtr.py's main() with --scene_mesh_field alone (it implies --register_scene) on the hand-made three-block split of
    tests/test_hip_render_scene.py.  Untrained weights: plumbing; the gt file is checked against scene_mesh under the known poses."""
    from dreg_nerf_amd import scene_reg, synth, vis_dump
    root, jd, res = tmp_path / "data", tmp_path / "json", 24
    T = {0: torch.eye(4), 1: synth.fixed_pose(), 3: synth.fixed_pose(1)}
    (root / "objaverse" / "images" / "sceneA").mkdir(parents=True)
    jd.mkdir()
    json.dump({str(k): v.tolist() for k, v in T.items()}, open(root / "objaverse" / "images" / "sceneA" / "world_frame_transforms.json", "w"))
    json.dump({"train": [], "test": ["sceneA"]}, open(jd / "objaverse.json", "w"))
    ck = []
    for n, k in enumerate(T):
        d = root / "objaverse" / "nerf_models" / "sceneA" / f"block_{k}"
        ck.append(str(d / "model.pth"))
        TS._write_checkpoint(ck[-1], four[n], TS.SCENE_CAMS[n])
        g, m = synth.shell_grid(32, 20 + k, *synth.shell_radii(32), pose=T[k])
        torch.save(g, d / "voxel_grid.pt")
        torch.save(m, d / "voxel_mask.pt")
    common = ["--root_dir", str(root), "--json_dir", str(jd), "--dataset", "objaverse", "--precision", "fp32", "--mesh_resolution", str(res)]
    TS._main(monkeypatch, common + ["--expname", "plain"])
    TS._main(monkeypatch, common + ["--expname", "field", "--scene_mesh_field"])
    text = capsys.readouterr().out
    assert "sceneA: scene field mesh of 3 blocks" in text and "scene_field_mesh_{aligned,gt}.ply" in text and "scene registration, 1 scenes" in text
    base = lambda name: str(root / "eval" / name / "objaverse")
    assert TPF._without_time(os.path.join(base("field"), "metrics_test.json")) == TPF._without_time(os.path.join(base("plain"), "metrics_test.json"))
    assert sorted(os.listdir(base("plain"))) == ["metrics_test.json"]
    assert sorted(os.listdir(base("field"))) == ["metrics_test.json", "sceneA", "scene_metrics_test.json"]
    d = os.path.join(base("field"), "sceneA")
    assert sorted(os.listdir(d)) == ["scene_field_mesh.json", "scene_field_mesh_aligned.ply", "scene_field_mesh_gt.ply"]
    stats = json.load(open(os.path.join(d, "scene_field_mesh.json")))
    assert set(stats) == {"K", "gt", "aligned", "level", "resolution", "power"}
    assert stats["K"] == 3 and stats["level"] == mesh.DENSITY_THRE and stats["resolution"] == res and stats["power"] == 4.0
    for name in ("gt", "aligned"):
        v, f, c, nrm = vis_dump.read_mesh_ply(os.path.join(d, f"scene_field_mesh_{name}.ply"))
        st = stats[name]
        assert set(st) == {"V", "F", "area", "volume"} and st["V"] == len(v) and st["F"] == len(f)
        if len(v):
            assert c.shape == v.shape and nrm.shape == v.shape and M.is_closed(f) and M.repeated_index_faces(f) == 0
            area, vol = mesh.mesh_area_volume(torch.from_numpy(v), torch.from_numpy(f))
            assert st["area"] == pytest.approx(area, rel=1e-12) and st["volume"] == pytest.approx(vol, rel=1e-12) and vol > 0 and area > 0
    assert stats["gt"]["V"] > 100 and stats["gt"]["F"] > 100
    # the gt file is scene_mesh of the three blocks under the known poses, the anchor under its own (the identity) as the renderer takes it
    scene = [{"nerf_path": p, "transform": T[k], "block_id": k} for p, k in zip(ck, T)]
    G = scene_reg.ground_truth(scene)
    loaded = [R.load_render_block(p, DEV) for p in ck]
    cen = [torch.as_tensor(b[2]["camera_poses"]).float()[:, :3, 3].mean(0) for b in loaded]
    m = S.scene_mesh(S.SceneField([(b[0], b[1], cen[i], G[i]) for i, b in enumerate(loaded)]), res)
    gt = vis_dump.read_mesh_ply(os.path.join(d, "scene_field_mesh_gt.ply"))
    assert np.array_equal(gt[0], m["verts"].cpu().numpy().astype(np.float64)) and np.array_equal(gt[1], m["faces"].cpu().numpy())
