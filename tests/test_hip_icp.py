"""GPU: the fused ICP kernels (csrc/icp.hip, dreg_nerf_amd/icp.py) against the fp64 restatement of their rule (tests/icp_restatement.py) on the
seeded cases of tests/icp_cases.py: exactly representable clouds (bit for bit), random clouds (correspondences up to the fp32 rounding of d^2,
sums within the counted roundings of e and J), convergence on the test solid, determinism, and the guards."""
import numpy as np
import pytest
import torch

import icp_cases as IC
import icp_restatement as IR
from dreg_nerf_amd import icp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
IDENTITY = IR.pose12_of(np.eye(3), np.zeros(3))


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _index(tgt, nrm, cell):
    return icp.TargetIndex(_dev(tgt), _dev(nrm), cell)


def _run(src, index, pose12, max_dist, iters, **kw):
    p = _dev(pose12, torch.float64)
    out = icp.refine_launch(_dev(src), index, p, max_dist, iters, kw.pop("tol_rot", 1e-7), kw.pop("tol_trans", 1e-7), **kw)
    torch.cuda.synchronize()
    return p.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


@pytest.mark.parametrize("ns", IC.EXACT_SIZES)
def test_exact_clouds_bit_for_bit(ns):
    """Lattice points, a 90 degree rotation, dyadic translation, axis normals: every fp32 product and every fp64 sum of the kernel is exact, so corr,
    dist2 and all 30 sums equal the fp64 restatement bit for bit, ties (planted and incidental) and zero normals included."""
    src, tgt, nrm = IC.exact_case(ns)
    index = _index(tgt, nrm, IC.EXACT_MAX_DIST)
    cid = IR.grid_of(tgt, IC.EXACT_MAX_DIST)[3]
    assert np.array_equal(index.cell_id.cpu().numpy(), cid)
    pose, got = _run(src, index, IC.EXACT_POSE, IC.EXACT_MAX_DIST, 1, want_sums=True, want_corr=True)
    corr, d2 = IR.correspondences(src, tgt, nrm, cid, IC.EXACT_POSE, IC.EXACT_MAX_DIST)
    want = IR.sums_given(src, tgt, nrm, corr, IC.EXACT_POSE)
    print(f"Ns {ns}: {int((corr >= 0).sum())} correspondences, sums[27:] {want[27:].tolist()}")
    assert np.array_equal(got["corr"], corr.astype(np.int32))
    assert np.array_equal(got["dist2"], d2.astype(np.float32)) and np.array_equal(got["dist2"].astype(np.float64), d2)
    assert np.array_equal(got["sums"], want)
    assert got["stats"][0, 0] == want[29] and got["stats"][0, 1] == want[27] and got["stats"][0, 2] == want[28]
    if ns >= 255:
        assert (corr >= 0).sum() >= 6 and (corr < 0).sum() > 0
    if want[29] < 6:
        assert got["stats"][0, 6] == 2 and np.array_equal(pose, IC.EXACT_POSE)


@pytest.mark.parametrize("seed", IC.RANDOM_SEEDS)
def test_random_clouds_match_the_brute_force_search(seed):
    """corr against the fp64 brute force.  A point is left out when fp32 rounding may decide it: the kernel's d^2 differs from the exact one by at
    most m = 2^-24 (12 sum_c |r_c| Q_c + 5 d^2), Q_c = sum_j |R_cj p_j| + |t_c| (icp_cases.d2_margin: six roundings on q_c, one on r_c, the squares
    and two sums), so the best and the runner-up can swap only when their exact d^2 differ by less than the sum of their margins, and the gate can
    flip only within m + 2 * 2^-24 max_dist^2 of max_dist^2.  At most 1 % of the points (asserted per seed on the CPU, tests/test_icp_host.py).
    The 30 sums, formed for the DEVICE's correspondences, stay within icp_cases.sums_bound (the fp32 roundings of e and J, counted there)."""
    src, tgt, nrm, pose = IC.random_case(seed)
    cell = icp.default_cell(IC.MAX_DIST)
    index = _index(tgt, nrm, cell)
    cid = IR.grid_of(tgt, cell)[3]
    _, got = _run(src, index, pose, IC.MAX_DIST, 1, want_sums=True, want_corr=True)
    corr, d2 = IR.correspondences(src, tgt, nrm, cid, pose, IC.MAX_DIST)
    amb = IC.ambiguous(src, tgt, cid, pose, IC.MAX_DIST)
    firm = ~amb
    print(f"seed {seed}: Ns {len(src)} Nt {len(tgt)}, {int((corr >= 0).sum())} correspondences, {int(amb.sum())} left out, "
          f"{int((got['corr'] != corr)[amb].sum())} of them differ")
    assert amb.mean() <= 0.01
    assert np.array_equal(got["corr"][firm], corr[firm].astype(np.int32))
    have = firm & (corr >= 0)
    assert np.all(np.abs(got["dist2"][have].astype(np.float64) - d2[have]) <= IC.d2_margin(src, tgt, np.where(corr >= 0, corr, 0), pose)[have] + 2.0 ** -24 * d2[have])
    dcorr = got["corr"].astype(np.int64)
    want, bound = IR.sums_given(src, tgt, nrm, dcorr, pose), IC.sums_bound(src, tgt, nrm, dcorr, pose)
    err = np.abs(got["sums"] - want)
    print("  largest |sum - restatement| / bound:", float((err[:29] / bound[:29]).max()))
    assert got["sums"][29] == want[29] and np.all(err <= bound)


@pytest.mark.parametrize("name", ["3deg", "6deg", "partial"])
def test_convergence_on_the_test_solid(name):
    src, tgt, nrm, R, t = IC.convergence_cases()[name]
    iters = IC.MAX_ITERS + 3
    pose, info = icp.refine_pose(_dev(src), _index(tgt, nrm, icp.default_cell(IC.MAX_DIST)), torch.eye(4), max_dist=IC.MAX_DIST, iters=iters)
    pose = pose.cpu().numpy()
    stats = info["stats"].numpy()
    rre, rte = IR.rre_deg(pose[:3, :3], R), IR.rte(pose[:3, 3], t)
    print(f"{name}: RRE {rre:.3e} deg, RTE {rte:.3e}, frozen after {info['iterations']} iterations, fitness {info['fitness']:.3f}, "
          f"|omega| per iteration {stats[:, 3].tolist()}")
    assert rre <= IC.RRE_BOUND_DEG and rte <= IC.RTE_BOUND
    assert info["status"] == 1 and info["iterations"] <= IC.MAX_ITERS
    k = info["iterations"] - 1
    assert all(np.array_equal(stats[j], stats[k]) for j in range(k, iters)) and np.all(stats[:k, 6] == 0)
    assert np.array_equal(pose[3], [0, 0, 0, 1]) and np.abs(pose[:3, :3] @ pose[:3, :3].T - np.eye(3)).max() < 1e-12
    assert stats[k, 0] == (703 if name == "partial" else len(src)) and info["fitness"] == stats[k, 0] / len(src)
    assert info["plane_rmse"] <= info["inlier_rmse"] + 1e-12


def test_two_runs_are_bit_identical():
    src, tgt, nrm, pose = IC.random_case(2)
    start = IR.pose12_of(pose[:9].reshape(3, 3) @ IC.rotation((1, 1, 0), 2.0), pose[9:] + 0.01)
    index = _index(tgt, nrm, icp.default_cell(IC.MAX_DIST))
    a = _run(src, index, start, IC.MAX_DIST, 5, want_sums=True, want_corr=True)
    b = _run(src, index, start, IC.MAX_DIST, 5, want_sums=True, want_corr=True)
    assert not np.array_equal(a[0], start)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


def test_too_few_and_degenerate_runs_leave_the_pose_bit_identical():
    pts, nrm = IC.test_solid(32)
    start = IR.pose12_of(IC.rotation((0, 0, 1), 0.5), [0.001, 0.002, -0.001])
    few = np.concatenate([pts[:5], pts[:300] + 10.0]).astype(np.float32)                 # two workgroups, five correspondences
    pose, got = _run(few, _index(pts, nrm, icp.default_cell(0.1)), start, 0.1, 3)
    assert np.array_equal(pose, start) and got["stats"][0, 0] == 5 and np.all(got["stats"][:, 6] == 2) and np.array_equal(got["stats"][2], got["stats"][0])
    tgt, pn, src = IC.tilted_plane()
    pose, got = _run(src, _index(tgt, pn, icp.default_cell(0.1)), start, 0.1, 3)
    print(f"tilted plane: count {got['stats'][0, 0]:.0f}, smallest pivot ratio {got['stats'][0, 5]:.3e}")
    assert np.array_equal(pose, start) and np.all(got["stats"][:, 6] == 3) and got["stats"][0, 0] > 300 and got["stats"][0, 5] <= 1e-6
    src, tgt, sn = IC.radial_sphere()
    pose, got = _run(src, _index(tgt, sn, icp.default_cell(0.1)), IDENTITY, 0.1, 2)
    assert np.array_equal(pose, IDENTITY) and np.all(got["stats"][:, 6] == 3) and got["stats"][0, 0] == 600 and got["stats"][0, 5] == 0.0
    p4, info = icp.refine_pose(_dev(few), _index(pts, nrm, icp.default_cell(0.1)), torch.eye(4), max_dist=0.1, iters=3)
    assert info["status"] == 2 and info["iterations"] == 1 and torch.equal(p4.cpu(), torch.eye(4, dtype=torch.float64))


def test_empty_source_and_a_cell_narrower_than_the_radius():
    pts, nrm = IC.test_solid(32)
    index = _index(pts, nrm, 0.1)
    pose, info = icp.refine_pose(torch.zeros(0, 3, device=DEV), index, torch.eye(4), max_dist=0.1, iters=2)
    assert info["status"] == 2 and info["fitness"] == 0.0 and info["iterations"] == 1 and torch.equal(pose.cpu(), torch.eye(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="narrower"):
        icp.refine_pose(_dev(pts), index, torch.eye(4), max_dist=0.11)
    # the library refuses it as well, before any launch
    from dreg_nerf_amd import lib as L
    lib = L.load()
    ws = torch.empty(lib.dreg_icp_workspace_bytes(len(pts), 1) // 8, dtype=torch.float64, device=DEV)
    p, st, s = _dev(IDENTITY, torch.float64), torch.zeros(1, 7, dtype=torch.float64, device=DEV), _dev(pts)
    args = [L.ptr(s), len(pts), L.ptr(index.points), L.ptr(index.normals), L.ptr(index.perm), L.ptr(index.cell_start), index.n, (L.c_float * 3)(*index.lo),
            index.cell, *index.dims, L.ptr(p)]
    tail = [1, 1e-7, 1e-7, 1e-6, L.ptr(st), None, None, None, L.ptr(ws), ws.numel() * 8, L.stream()]
    assert lib.dreg_icp_refine(*args, 0.2, *tail) == -1
    assert lib.dreg_icp_refine(*args[:-1], None, 0.05, *tail) == -1
    assert lib.dreg_icp_refine(*args, 0.05, *tail[:-2], 8, L.stream()) == -1                       # workspace too small
    assert lib.dreg_icp_refine(*args, 0.05, *tail) == 0
    torch.cuda.synchronize()
    assert st[0, 0].item() == len(pts)


def test_block_normals_without_a_field_are_the_pca_normals():
    pts, nrm = IC.test_solid(32)
    n = icp.block_normals(_dev(pts)).cpu().numpy()
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-4
