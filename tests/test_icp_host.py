"""CPU: the rule of the ICP refinement (tests/icp_restatement.py) and of the density gradient (tests/ngp_grad_restatement.py) on their own, the target
index of dreg_nerf_amd/icp.py against a brute-force search, the seeded cases of tests/icp_cases.py that the device tests rely on, and the
evaluator's files for --refine_pose with an injected refiner.  The kernels themselves: tests/test_hip_icp.py, tests/test_hip_ngp_grad.py."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import icp_cases as IC
import icp_restatement as IR
import ngp_grad_restatement as GR
from dreg_nerf_amd import icp, vis_dump

IDENTITY = IR.pose12_of(np.eye(3), np.zeros(3))


def test_solid_has_the_stated_size_and_unit_axis_normals():
    pts, nrm = IC.test_solid(32)
    assert pts.shape == (1492, 3) and pts.dtype == np.float32
    assert np.all(np.abs(nrm).sum(axis=1) == 1.0) and set(np.unique(nrm)) == {-1.0, 0.0, 1.0}
    cases = IC.convergence_cases()
    assert (len(cases["partial"][0]), len(cases["partial"][1])) == (1036, 1103)


@pytest.mark.parametrize("name", ["3deg", "6deg", "partial"])
@pytest.mark.parametrize("kernel_arithmetic", [False, True], ids=["fp64", "fp32_points"])
def test_restatement_recovers_the_known_pose(name, kernel_arithmetic):
    """Both in fp64 throughout and with q, e, J formed in fp32 as the kernel forms them: the fp32 floor is below the thresholds of the device test."""
    src, tgt, nrm, R, t = IC.convergence_cases()[name]
    pose, stats = IR.refine(src, tgt, nrm, IDENTITY, IC.MAX_DIST, IC.MAX_ITERS, kernel_arithmetic=kernel_arithmetic)
    rre, rte = IR.rre_deg(pose[:9].reshape(3, 3), R), IR.rte(pose[9:], t)
    print(f"{name}: RRE {rre:.3e} deg, RTE {rte:.3e}, status per iteration {stats[:, 6].tolist()}, count {stats[-1, 0]:.0f}")
    assert rre <= IC.RRE_BOUND_DEG and rte <= IC.RTE_BOUND
    assert stats[-1, 6] == 1                                    # converged and frozen within the 6 iterations
    frozen = int(np.nonzero(stats[:, 6])[0][0])
    assert all(np.array_equal(stats[k], stats[frozen]) for k in range(frozen, IC.MAX_ITERS))
    if name == "partial":
        assert stats[-1, 0] == 703
    else:
        assert stats[-1, 0] == len(src)


def _index(tgt, nrm, cell):
    return icp.TargetIndex(torch.from_numpy(np.ascontiguousarray(tgt)), torch.from_numpy(np.ascontiguousarray(nrm)), cell)


def test_target_index_layout_matches_the_restatement():
    _, tgt, nrm, _ = IC.random_case(1)
    ix = _index(tgt, nrm, icp.default_cell(IC.MAX_DIST))
    lo, cell, dims, cid = IR.grid_of(tgt, icp.default_cell(IC.MAX_DIST))
    assert ix.dims == dims and ix.cell == cell and np.array_equal(np.array(ix.lo, dtype=np.float32), lo)
    assert np.array_equal(ix.cell_id.numpy(), cid)
    perm, start = ix.perm.numpy(), ix.cell_start.numpy()
    assert start.dtype == np.int32 and len(start) == dims[0] * dims[1] * dims[2] + 1 and start[0] == 0 and start[-1] == len(tgt)
    assert np.array_equal(perm, np.lexsort((np.arange(len(tgt)), cid)))                    # stable: ascending (cell id, caller index)
    assert np.array_equal(ix.points.numpy(), tgt[perm]) and np.array_equal(ix.normals.numpy(), nrm[perm])
    sorted_cid = cid[perm]
    assert all(np.all(sorted_cid[start[c]:start[c + 1]] == c) for c in np.unique(cid))
    # one empty cell on every side: the last one exactly; the first up to the rounding of lo = min - cell (the smallest coordinate may land on
    # the upper face of cell 0 instead of the lower face of cell 1: still a cell's width, less that rounding, from the grid's edge)
    key = np.stack([cid % dims[0], (cid // dims[0]) % dims[1], cid // (dims[0] * dims[1])], axis=1)
    assert all(key[:, c].max() == dims[c] - 2 for c in range(3)) and key.min() >= 0
    assert ((tgt.astype(np.float64) - lo.astype(np.float64)) >= cell * (1 - 2.0 ** -20)).all()


def test_grid_with_too_many_cells_doubles_the_cell():
    tgt = np.array([[0, 0, 0], [100, 100, 100], [50, 3, 7]], dtype=np.float32)
    ix = _index(tgt, np.ones_like(tgt), 0.05)
    doublings = math.log2(ix.cell / float(np.float32(0.05)))
    assert ix.dims[0] * ix.dims[1] * ix.dims[2] <= 1 << 24 and doublings == round(doublings) and doublings >= 1
    half = ix.cell / 2                                                        # one doubling less would not have fitted
    assert np.prod([math.floor(100 / half) + 3 for _ in range(3)]) > 1 << 24
    assert IR.grid_of(tgt, 0.05)[1:3] == (ix.cell, ix.dims)


@pytest.mark.parametrize("seed", [0, 1])
def test_27_cell_scan_is_the_brute_force_nearest_neighbour(seed):
    """Dense random clouds (several points per cell), target points on the faces of the grid's cells, source points outside the grid and duplicates
    of target points: the index plus the kernel's scan (icp_cases.scan27) returns exactly the brute-force nearest neighbour within max_dist."""
    rng = np.random.default_rng(seed)
    max_dist = 0.1
    cell = icp.default_cell(max_dist)
    tgt = rng.uniform(-0.5, 0.5, (3000, 3)).astype(np.float32)                  # 10 cells per axis: about 3 points per cell
    lo0 = tgt.min(axis=0) - np.float32(cell)
    on_face = (lo0 + np.float32(cell) * rng.integers(1, 9, (300, 3)).astype(np.float32)).astype(np.float32)
    on_face[:, 1:] += rng.uniform(0, 0.3, (300, 2)).astype(np.float32)          # x on a face, y / z free
    tgt = np.concatenate([tgt, on_face, tgt[:50]])                               # and 50 duplicates (ties by caller index)
    nrm = np.ones_like(tgt)
    nrm[rng.integers(0, 10, len(tgt)) == 0] = 0.0
    ix = _index(tgt, nrm, cell)
    q = np.concatenate([rng.uniform(-0.8, 0.8, (1500, 3)), tgt[:200].astype(np.float64), on_face[:100] + [[max_dist * 0.999, 0, 0]],
                        rng.uniform(-3, 3, (100, 3)), [[np.nan, 0, 0], [1e30, 0, 0]]]).astype(np.float32)
    got_i, got_d = IC.scan27(ix, q, max_dist)
    # brute force in the same fp32 arithmetic, ties to the smallest (cell id, caller index)
    order = np.lexsort((np.arange(len(tgt)), ix.cell_id.numpy()))
    ts = tgt[order]
    want_i = np.full(len(q), -1, dtype=np.int64)
    want_d = np.full(len(q), np.inf, dtype=np.float32)
    md2 = np.float32(max_dist) * np.float32(max_dist)
    for i, qi in enumerate(q):
        r = qi[None] - ts
        d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        if np.isnan(d2).any():
            continue
        j = int(np.argmin(d2))
        if d2[j] <= md2 and nrm[order[j]].any():
            want_i[i], want_d[i] = order[j], d2[j]
    assert (want_i >= 0).sum() > 500 and (want_i < 0).sum() > 100
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)


def _plane(n=400, seed=0):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], axis=1).astype(np.float32)
    return p, np.tile(np.array([[0, 0, 1]], dtype=np.float32), (n, 1))


def test_single_plane_is_degenerate_and_keeps_the_pose():
    """Axis-aligned, J has zero columns (a zero diagonal counts as degenerate); in general position no diagonal entry vanishes and a pivot falls
    to rounding level against its diagonal entry."""
    tgt, nrm = _plane()
    src = (tgt + np.array([0.0, 0.0, 0.01], dtype=np.float32)).astype(np.float32)
    pose, stats = IR.refine(src, tgt, nrm, IDENTITY, 0.1, 3)
    assert stats[0, 6] == 3 and np.array_equal(pose, IDENTITY) and np.array_equal(stats[1], stats[0]) and stats[0, 5] == 0.0
    tgt2, nrm2, src2 = IC.tilted_plane()
    pose, stats = IR.refine(src2, tgt2, nrm2, IDENTITY, 0.1, 3)
    print(f"tilted plane: smallest pivot ratio {stats[0, 5]:.3e}")
    assert stats[0, 6] == 3 and np.array_equal(pose, IDENTITY) and 0.0 < abs(stats[0, 5]) <= 1e-6 and stats[0, 0] == len(src2)


def test_fewer_than_six_correspondences_is_status_2():
    pts, nrm = IC.test_solid(32)
    src = np.concatenate([pts[:5], pts[:40] + 10.0]).astype(np.float32)         # five near, the rest far beyond the gate
    pose, stats = IR.refine(src, pts, nrm, IDENTITY, 0.1, 2)
    assert stats[0, 0] == 5 and stats[0, 6] == 2 and np.array_equal(pose, IDENTITY)


def test_sphere_with_radial_normals_is_degenerate():
    """q x n = 0 for every pair when q is (nearly) radial: the rotation block of J^T J vanishes."""
    src, tgt, nrm = IC.radial_sphere()
    pose, stats = IR.refine(src, tgt, nrm, IDENTITY, 0.1, 2)
    assert stats[0, 0] == 600 and stats[0, 6] == 3 and np.array_equal(pose, IDENTITY)


def test_exponential_map_closed_forms():
    assert np.array_equal(IR.exp_so3([0, 0, 0]), np.eye(3))
    for axis in range(3):
        for th in (1e-9, 1e-4, 0.3, math.pi / 2, 3.0):
            w = np.zeros(3)
            w[axis] = th
            a, b = (axis + 1) % 3, (axis + 2) % 3
            want = np.eye(3)
            want[a, a] = want[b, b] = math.cos(th)
            want[b, a], want[a, b] = math.sin(th), -math.sin(th)
            assert np.abs(IR.exp_so3(w) - want).max() <= 4e-16
    rng = np.random.default_rng(0)
    for _ in range(20):
        w = rng.normal(size=3) * rng.uniform(1e-8, 3)
        E = IR.exp_so3(w)
        assert np.abs(E @ E.T - np.eye(3)).max() <= 4e-15 and abs(np.linalg.det(E) - 1) <= 4e-15
        assert np.abs(E @ w - w).max() <= 4e-15 * max(1.0, np.abs(w).max())       # the axis is fixed
        assert abs((np.trace(E) - 1) / 2 - math.cos(np.linalg.norm(w))) <= 4e-15


@pytest.mark.parametrize("seed", IC.RANDOM_SEEDS)
def test_random_cases_leave_out_at_most_one_percent(seed):
    src, tgt, nrm, pose = IC.random_case(seed)
    assert 1000 <= len(src) <= 3000 and 1000 <= len(tgt) <= 3000
    cid = IR.grid_of(tgt, icp.default_cell(IC.MAX_DIST))[3]
    amb = IC.ambiguous(src, tgt, cid, pose, IC.MAX_DIST)
    corr, _ = IR.correspondences(src, tgt, nrm, cid, pose, IC.MAX_DIST)
    print(f"seed {seed}: Ns {len(src)}, Nt {len(tgt)}, {int((corr >= 0).sum())} correspondences, {int(amb.sum())} ambiguous")
    assert amb.mean() <= 0.01 and (corr >= 0).mean() > 0.3 and (corr < 0).mean() > 0.05


@pytest.mark.parametrize("ns", IC.EXACT_SIZES)
def test_exact_cases_are_exact_and_have_ties(ns):
    src, tgt, nrm = IC.exact_case(ns)
    q = IR.transform(src, IC.EXACT_POSE) * 32.0
    assert np.array_equal(q, np.round(q)) and np.array_equal(tgt * 32.0, np.round(tgt * 32.0))            # all on the 2^-5 lattice
    cid = IR.grid_of(tgt, IC.EXACT_MAX_DIST)[3]
    _, d1, d2 = IR.nearest(src, tgt, cid, IC.EXACT_POSE)
    assert (d1[:min(ns, 8)] == d2[:min(ns, 8)]).all()                                                       # the planted midpoints tie
    if ns >= 255:
        assert (nrm == 0).all(axis=1).any() and (d1 == d2).sum() >= 8


# ------------------------------------------------------------------------------------------------------------------ evaluator files
def test_refine_flag_files_and_schema_with_an_injected_refiner(tmp_path):
    import eval_nerf_regtr as EV
    g = torch.Generator().manual_seed(0)
    src, tgt = torch.rand(300, 3, generator=g), torch.rand(320, 3, generator=g)
    gt = torch.eye(4)[None]
    pred = {"pose": torch.eye(4)[:3][None, None].repeat(6, 1, 1, 1)}
    pred["pose"][-1, 0, :, 3] = torch.tensor([0.1, 0.0, 0.0])
    cfg = types.SimpleNamespace(icp_normals="field", icp_max_dist=0.05, icp_iters=30)
    seen, lines = {}, []

    def refiner(s, index, pose4, max_dist, iters):
        seen.update(ns=s.shape[0], nt=index.n, cell=index.cell, pose=pose4.clone(), max_dist=max_dist, iters=iters,
                    unit=bool(((index.normals.norm(dim=1) - 1).abs() < 1e-4).all()))
        return torch.eye(4, dtype=torch.float64), {"status": seen.get("status", 1), "fitness": 0.5, "iterations": 3}

    rows, refined = {}, {}
    for k, status in (("a", 1), ("b", 3)):
        seen["status"] = status
        data = {"scene": k, "pose": gt, "src_sparse": types.SimpleNamespace(vals=torch.cat([src, src], dim=1)),
                "tgt_sparse": types.SimpleNamespace(vals=torch.cat([tgt, tgt], dim=1)), "tgt_nerf_path": str(tmp_path / "missing.pth")}
        rows[k] = EV._row({"R_error_mean": 0.0, "t_error_mean": 0.1, "R_error_med": 0.0, "t_error_med": 0.1}, 0.01)
        refined[k] = EV.refine_scene_pose(cfg, data, pred, torch.device("cpu"), refiner=refiner, log=lambda m, **kw: lines.append(m))
    assert seen["ns"] == 300 and seen["nt"] == 320 and seen["max_dist"] == 0.05 and seen["iters"] == 30 and seen["unit"] and seen["cell"] >= 0.05
    assert torch.equal(seen["pose"][:3], pred["pose"][-1, 0]) and seen["pose"].shape == (4, 4)
    assert len(lines) == 2 and all("PCA" in m for m in lines)                       # no block on disk: said so, per scene
    assert refined["a"]["t_mean"] == 0.0 and refined["a"]["status"] == 1            # the refiner's pose (the ground truth) was scored
    assert abs(refined["b"]["t_mean"] - 0.1) < 1e-6 and refined["b"]["status"] == 3  # degenerate: the predicted pose is kept
    out = EV.write_refined(str(tmp_path), "test", rows, refined, log=lambda m, **kw: lines.append(m))
    on_disk = json.load(open(tmp_path / "refined_metrics_test.json"))
    assert on_disk == out and set(on_disk) == {"a", "b", "R_mean", "t_mean"}
    assert set(on_disk["a"]) == {"R_mean", "t_mean", "R_med", "t_med", "time", "fitness", "status"}
    assert abs(on_disk["t_mean"] - 0.05) < 1e-6 and "0.1000 -> 0.0500" in lines[-1]
    assert os.listdir(tmp_path) == ["refined_metrics_test.json"]                    # metrics_{split}.json is not this code's to touch


def test_write_ply_bytes_are_unchanged_without_normals(tmp_path):
    rng = np.random.default_rng(0)
    xyz, rgb, nrm = rng.normal(size=(7, 3)), rng.uniform(size=(7, 3)), rng.normal(size=(7, 3))
    head = "ply\nformat binary_little_endian 1.0\ncomment Created by dreg_nerf_amd (open3d point-cloud layout)\nelement vertex 7\nproperty double x\nproperty double y\nproperty double z\n"
    vis_dump.write_ply(str(tmp_path / "a.ply"), xyz)
    assert open(tmp_path / "a.ply", "rb").read() == (head + "end_header\n").encode() + xyz.astype("<f8").tobytes()
    vis_dump.write_ply(str(tmp_path / "b.ply"), xyz, rgb)
    rec = np.empty(7, dtype=[("p", "<f8", 3), ("c", "u1", 3)])
    rec["p"], rec["c"] = xyz, np.clip(np.round(rgb * 255.0), 0, 255).astype(np.uint8)
    assert open(tmp_path / "b.ply", "rb").read() == (head + "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode() + rec.tobytes()
    vis_dump.write_ply(str(tmp_path / "c.ply"), xyz, rgb, nrm)
    p, n, c = vis_dump.read_ply_normals(str(tmp_path / "c.ply"))
    assert np.array_equal(p, xyz) and np.array_equal(n, nrm) and np.array_equal(c, rec["c"])
    assert b"property double z\nproperty double nx\nproperty double ny\nproperty double nz\nproperty uchar red" in open(tmp_path / "c.ply", "rb").read()
    vis_dump.write_ply(str(tmp_path / "d.ply"), xyz, None, nrm)
    p, n, c = vis_dump.read_ply_normals(str(tmp_path / "d.ply"))
    assert np.array_equal(p, xyz) and np.array_equal(n, nrm) and c is None


def test_pca_normals_in_chunks_equal_the_dense_form():
    from dreg_nerf_amd import fgr
    pts, nrm = IC.test_solid(32)
    p = torch.from_numpy(pts)
    a, b = icp.pca_normals(p, 0.15, 30, chunk=100), fgr.estimate_normals(p, 0.15, 30)
    assert torch.allclose(a, b, atol=1e-5)
    flat = (np.abs(nrm).sum(axis=1) == 1)                                         # away from edges the PCA normal is the face's axis, up to sign
    dots = (a.numpy() * nrm).sum(axis=1)
    assert np.median(np.abs(dots[flat])) > 0.99


# ------------------------------------------------------------------------------------------------------------------ density gradient rule
def small_field(seed=0, n_levels=4, hidden=8):
    """A small field for the gradient restatement: two dense levels, two hashed ones; weights of order one."""
    rng = np.random.default_rng(seed)
    res = np.array([4, 7, 12, 20], dtype=np.uint32)[:n_levels]
    size = np.array([64, 344, 512, 512], dtype=np.uint32)[:n_levels]
    lv = {"res": res, "size": size, "scale": (res.astype(np.float32) - np.float32(1.3)), "hashed": (res.astype(np.int64) ** 3 > size).astype(np.uint32),
          "offset": np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)}
    table = rng.uniform(-0.5, 0.5, (int(size.sum()), 2))
    w1 = rng.uniform(-0.6, 0.6, (hidden, 2 * n_levels))
    w2 = rng.uniform(-0.6, 0.6, (3, hidden))
    aabb = np.array([-1.0, -0.5, 0.0, 1.0, 1.5, 3.0], dtype=np.float32)
    return lv, table, w1, w2, aabb


def test_gradient_restatement_equals_central_differences_of_its_fp64_forward():
    lv, table, w1, w2, aabb = small_field()
    assert lv["hashed"].tolist() == [0, 0, 1, 1]
    rng = np.random.default_rng(1)
    x = (aabb[:3] + (aabb[3:] - aabb[:3]) * rng.uniform(0.02, 0.98, (4000, 3))).astype(np.float32)
    h = 1e-6
    sigma, mask, pre = GR.forward64(x, table, w1, w2, lv, aabb)
    keep = (GR.face_distance(x, lv, aabb) > 4 * h) & (np.abs(pre).min(axis=1) > 1e-3)         # away from every cell face and every ReLU kink
    assert keep.sum() > 2000
    x, sigma, mask = x[keep], sigma[keep], mask[keep]
    grad, M = GR.density_grad(x, table, w1, w2, lv, aabb, sigma, mask, coords=np.float64)
    fd = np.zeros_like(grad)
    for c in range(3):
        e = np.zeros(3)
        e[c] = h
        fd[:, c] = (GR.forward64(x.astype(np.float64) + e, table, w1, w2, lv, aabb)[0] - GR.forward64(x.astype(np.float64) - e, table, w1, w2, lv, aabb)[0]) / (2 * h)
    # relative to the gradient's own scale M (the sum of the absolute terms): central differences of an analytic function with h = 1e-6 carry
    # h^2 f''' / 6 truncation and eps f / h ~ 1e-10 rounding, both far below 1e-6 M
    live = M > 0                                           # M == 0: no hidden unit is active, the field is locally constant
    assert live.all(axis=1).mean() > 0.9 and np.abs(fd[~live]).max(initial=0.0) <= 1e-9 and np.abs(grad[~live]).max(initial=0.0) == 0.0
    rel = np.abs(grad - fd)[live] / M[live]
    print(f"{keep.sum()} points, max |grad - fd| / M = {rel.max():.2e}, median |grad| / M = {np.median(np.abs(grad)[live] / M[live]):.2e}")
    assert rel.max() <= 1e-6


def test_gradient_restatement_is_zero_outside_and_mask_bits_round_trip():
    lv, table, w1, w2, aabb = small_field()
    x = np.array([[-1.0, 0.0, 1.0], [2.0, 0.0, 1.0], [0.0, 0.5, 3.0], [0.0, 0.5, 1.0]], dtype=np.float32)      # on a face, outside, on a face, inside
    sigma, mask, _ = GR.forward64(x, table, w1, w2, lv, aabb)
    assert sigma[:3].tolist() == [0.0, 0.0, 0.0] and sigma[3] > 0
    grad, _ = GR.density_grad(x, table, w1, w2, lv, aabb, np.ones(4), mask)
    assert np.array_equal(grad[:3], np.zeros((3, 3))) and np.abs(grad[3]).max() > 0
    bits = np.array([0, 1, (1 << 63) | 5, (1 << 64) - 1], dtype=np.uint64)
    m = GR.mask_bits(bits)
    assert m.shape == (4, 64) and m[1].sum() == 1 and m[1, 0] and m[2, 63] and m[2, 0] and m[2, 2] and m[2].sum() == 3 and m[3].all()
    assert np.array_equal(GR.mask_bits(bits.astype(np.int64)), m)                              # torch hands the mask over as int64 bits
