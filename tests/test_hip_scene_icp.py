"""GPU: the joint K-block ICP kernels (csrc/icp_scene.hip, dreg_nerf_amd/scene_icp.py) — per pair the 30 sums of the pair kernel bit for bit,
the solve against the fp64 restatement (tests/scene_icp_restatement.py) within a counted bound, convergence on partial views of the test solid,
determinism, the guards, and eval_nerf_regtr.py --refine_scene end to end."""
import json
import math
import os

import numpy as np
import pytest
import torch

import icp_cases as IC
import icp_restatement as IR
import scene_icp_cases as SC
import scene_icp_restatement as SR
from dreg_nerf_amd import icp, scene_icp
from dreg_nerf_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _scene(points, normals, cell):
    pts = [_dev(p) for p in points]
    return pts, [icp.TargetIndex(p, _dev(n), cell) for p, n in zip(pts, normals)]


def _run(pts, idx, G12, max_dist, iters, **kw):
    p = _dev(G12, torch.float64)
    out = scene_icp.refine_launch(pts, idx, p, max_dist, iters, kw.pop("tol_rot", 1e-7), kw.pop("tol_trans", 1e-7), want_pair_sums=True, want_rel=True, **kw)
    torch.cuda.synchronize()
    return p.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def _pair_kernel_sums(pts, idx, rel, i, j, max_dist):
    """The pair kernel's `sums` on (block i's points, block j's index, the device's own rel[i][j])."""
    out = icp.refine_launch(pts[i], idx[j], _dev(rel[i, j], torch.float64), max_dist, 1, 1e-7, 1e-7, want_sums=True)
    torch.cuda.synchronize()
    return out["sums"].cpu().numpy(), out["stats"].cpu().numpy()[0]


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("sizes", SC.SCENE_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_pair_sums_equal_the_pair_kernel_bit_for_bit(sizes, kind, holes):
    K = len(sizes)
    if kind == "exact":
        points, normals, G12 = SC.exact_scene(sizes)
        max_dist = cell = SC.EXACT_MAX_DIST
    else:
        points, normals, G12 = SC.random_scene(sizes)
        G12 = G12.copy()
        for b in range(1, K):                                # off the true poses: 1 degree and 0.01
            G12[b] = SR.perturbed(G12[b], np.array([0.01, -0.012, 0.005, 0.006, -0.005, 0.006]))
        max_dist, cell = IC.MAX_DIST, icp.default_cell(IC.MAX_DIST)
    mask = SC.holed_mask(K) if holes else None
    pts, idx = _scene(points, normals, cell)
    G_out, got = _run(pts, idx, G12, max_dist, 1, pair_mask=mask)
    pairs = SR.enabled_pairs(K, mask)
    tot = np.zeros(3)
    for i in range(K):
        for j in range(K):
            if (i, j) not in pairs:
                assert not got["pair_sums"][i, j].any(), (i, j)          # masked pairs and the diagonal: exactly zero
                continue
            sums, row = _pair_kernel_sums(pts, idx, got["rel"], i, j, max_dist)
            assert np.array_equal(got["pair_sums"][i, j], sums), (i, j)
            tot += [sums[29], sums[27], sums[28]]
    print(f"{sizes} {kind} holes={holes}: counts {[int(got['pair_sums'][i, j, 29]) for i, j in pairs]}, status {got['stats'][0, 6]:.0f}")
    # the totals: the pairs' values added in ascending (i, j) order, as the solve adds them
    assert np.array_equal(got["stats"][0, :3], tot)
    assert np.array_equal(G_out[0], G12[0])
    rel = SR.rel_poses(G12)
    if kind == "exact":
        assert np.array_equal(got["rel"], rel)
        corrs = SR.pair_correspondences(points, normals, SR.cell_ids(points, cell), rel, max_dist, mask)
        assert np.array_equal(got["pair_sums"], SR.pair_sums(points, normals, corrs, rel))
        assert sum(int((c >= 0).sum()) for c in corrs.values()) > 0 or min(sizes) == 1
    else:
        assert np.abs(got["rel"] - rel).max() <= 8 * 2.0 ** -53 * 2.0     # the same operations in the same order (sin / cos free): equal, or an ulp


def _recover_xi(G_new, G_old):
    """xi with G_new = exp(xi) G_old, per free block: omega from the skew part of E = R_new R_old^T (sin(th)/th omega), v = t_new - E t_old."""
    out = []
    for a, b in zip(G_new[1:], G_old[1:]):
        E = a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T
        w = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
        s = np.linalg.norm(w)
        w = w * (math.asin(s) / s if s > 0 else 1.0)
        out.append(np.concatenate([w, a[9:] - E @ b[9:]]))
    return np.concatenate(out)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_solve_against_the_restatement_fed_the_devices_sums(K):
    """One iteration on K views of the test solid, seen from a moved anchor frame, from a start near the true poses.  The restatement assembles and solves from the DEVICE's pair_sums and poses,
    so only the assembly and the solve differ.  Bound: |d xi|_inf <= c cond_2(H) 2^-53 |xi|_inf, c counted per implementation (the device and the
    restatement both round, hence the leading 2) from the kernel's operations at n = 6 (K - 1):
      adjoint products  every entry of A = M^T (A' M) is a 6-term sum of 6-term sums (12 roundings) and is added into H next to at most
                        2 (K - 1) - 1 <= 5 others, b = M^T b' likewise with 6 + 5: (17 mH + 11 mg) u, where mH = |sum |M^T| |A'| |M||_inf / |H|_inf and
                        mg = |sum |M^T| |b'||_inf / |g|_inf say how much larger the summed magnitudes are than the results (computed below from
                        the sums: properties of the data);
      factorisation and the two triangular solves  the classical (3 n + 1) u |L| |L^T| backward error, | |L| |L^T| |_2 <= n |H|_2: n (3 n + 1) u;
    and sqrt(n) for stating a 2-norm bound in the infinity norm: c = 2 sqrt(n) (n (3 n + 1) + 17 mH + 11 mg).  The device hands back poses, not
    xi: xi is recovered from exp(xi) = G_new G_old^-1, which with the update's own roundings (E from 3 operations per entry, E R and E t + v
    from 5 and 6) adds at most 32 * 2^-53 (1 + |t|) — stated apart, it does not scale with cond."""
    points, normals, G_true = SC.view_case(K)
    cell = icp.default_cell(IC.MAX_DIST)
    pts, idx = _scene(points, normals, cell)
    # every pose, the anchor's included, under one common motion of 40 degrees and |t| = 0.7: the same scene in another anchor frame, so that no
    # adjoint is the identity; the free blocks start 1 degree / 0.01 off their true poses
    T = SR.poses44_of([IR.pose12_of(IC.rotation((0.2, 0.9, -0.4), 40.0), [0.5, -0.3, 0.4])])[0]
    G0 = SR.poses12_of(T[None] @ SR.poses44_of(G_true))
    for b in range(1, K):
        G0[b] = SR.perturbed(G0[b], np.array([0.01, -0.012, 0.005, 0.006, -0.005, 0.006]) * (1 if b % 2 else -1))
    G_dev, got = _run(pts, idx, G0, IC.MAX_DIST, 1)
    pairs = SR.enabled_pairs(K)
    assert np.array_equal(G_dev[0], G0[0]) and np.abs(got["rel"] - SR.rel_poses(G0)).max() <= 2.0 ** -50
    H, g, tot = SR.assemble(got["pair_sums"], G0, pairs)
    G_ref, row, xi = SR.solve(H, g, tot, G0)
    assert row[6] == 0 and got["stats"][0, 6] == 0 and np.array_equal(got["stats"][0, :3], row[:3])
    n = 6 * (K - 1)
    Ha, ga = np.zeros_like(H), np.zeros_like(g)
    for i, j in pairs:
        A1, b1 = SR.unpack(got["pair_sums"][i, j])
        M = np.abs(SR.adjoint_inv(G0[j]))
        Aa, ba = M.T @ np.abs(A1) @ M, M.T @ np.abs(b1)
        for r in (i, j):
            ga[6 * r:6 * r + 6] += ba
            for s in (i, j):
                Ha[6 * r:6 * r + 6, 6 * s:6 * s + 6] += Aa
    mH, mg = Ha[6:, 6:].sum(axis=1).max() / np.abs(H[6:, 6:]).sum(axis=1).max(), ga[6:].max() / np.abs(g[6:]).max()      # of the reduced system
    c = 2.0 * math.sqrt(n) * (n * (3 * n + 1) + 17.0 * mH + 11.0 * mg)
    cond = np.linalg.cond(H[6:, 6:])
    bound = c * cond * 2.0 ** -53 * np.abs(xi).max() + 32 * 2.0 ** -53 * (1.0 + np.abs(G_dev[:, 9:]).max())
    err = np.abs(_recover_xi(G_dev, G0) - xi).max()
    line = f"K {K}: |d xi|_inf {err:.3e}, bound {bound:.3e} (c {c:.0f}, mH {mH:.2f}, mg {mg:.2f}, cond_2 {cond:.1f}, |xi|_inf {np.abs(xi).max():.3e}), ratio {err / bound:.3e}"
    print(line)                                              # profiles/scene_icp_ratios.txt holds these lines of the recorded run
    assert err <= bound
    assert np.abs(G_dev - G_ref).max() <= bound * (1.0 + np.abs(G0).max()) + 32 * 2.0 ** -53
    assert np.array_equal(got["stats"][0, 3:5] > 0, [True, True]) and abs(got["stats"][0, 5] - row[5]) <= 1e-9 * row[5]


@pytest.mark.parametrize("K", [3, 4])
def test_convergence_on_views_of_the_test_solid(K):
    points, normals, G_true = SC.view_case(K)
    pts, idx = _scene(points, normals, icp.default_cell(IC.MAX_DIST))
    iters = IC.MAX_ITERS + 3
    G0 = torch.eye(4, dtype=torch.float64).repeat(K, 1, 1)
    G, info = scene_icp.refine_poses(pts, idx, G0, max_dist=IC.MAX_DIST, iters=iters)
    G = G.cpu().numpy()
    stats = info["stats"].numpy()
    G12 = SR.poses12_of(G)
    rre, rte = SC.worst_errors(G12, G_true)
    print(f"K {K}: worst RRE {rre:.3e} deg, worst RTE {rte:.3e}, frozen after {info['iterations']} iterations, fitness {info['fitness']:.3f}, "
          f"max |omega| per iteration {stats[:, 3].tolist()}")
    assert rre <= IC.RRE_BOUND_DEG and rte <= IC.RTE_BOUND
    assert info["status"] == 1 and info["iterations"] <= IC.MAX_ITERS
    k = info["iterations"] - 1
    assert all(np.array_equal(stats[j], stats[k]) for j in range(k, iters)) and np.all(stats[:k, 6] == 0)
    assert np.array_equal(G[0], np.eye(4)) and np.all(G[:, 3] == [0, 0, 0, 1])
    assert max(np.abs(G[b, :3, :3] @ G[b, :3, :3].T - np.eye(3)).max() for b in range(K)) < 1e-12
    n_src = sum(len(points[i]) for i, _ in SR.enabled_pairs(K))
    assert info["fitness"] == stats[k, 0] / n_src and info["plane_rmse"] <= info["inlier_rmse"] + 1e-12


def test_two_runs_are_bit_identical_and_failures_leave_the_poses_alone():
    points, normals, _ = SC.view_case(3)
    cell = icp.default_cell(IC.MAX_DIST)
    pts, idx = _scene(points, normals, cell)
    start = SC.identity_poses(3).copy()
    start[1] = SR.perturbed(start[1], np.array([0.002, 0.001, -0.003, 0.001, 0.002, -0.001]))
    a = _run(pts, idx, start, IC.MAX_DIST, 5)
    b = _run(pts, idx, start, IC.MAX_DIST, 5)
    assert not np.array_equal(a[0][1:], start[1:]) and np.array_equal(a[0][0], start[0])
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    # a block beyond the gate of all others: status 3 through its zero diagonal
    far = [points[0], points[1], points[2] + np.float32(10.0)]
    fp, fi = _scene(far, normals, cell)
    G, got = _run(fp, fi, start, IC.MAX_DIST, 3)
    assert np.array_equal(G, start) and np.all(got["stats"][:, 6] == 3) and got["stats"][0, 0] > 12 and np.array_equal(got["stats"][2], got["stats"][0])
    assert not got["pair_sums"][2].any() and not got["pair_sums"][:, 2].any()
    # fewer than 6 (K - 1) = 12 correspondences: status 2
    few = [np.concatenate([points[0][:3], points[0][3:300] + np.float32(10.0)]), points[0][:2], points[0][:1]]
    fn = [normals[0][:300], normals[0][:2], normals[0][:1]]
    wp, wi = _scene(few, fn, icp.default_cell(0.01))
    G, got = _run(wp, wi, start, 0.01, 3)
    assert np.array_equal(G, start) and np.all(got["stats"][:, 6] == 2) and 0 <= got["stats"][0, 0] < 12
    G4, info = scene_icp.refine_poses(wp, wi, torch.eye(4).repeat(3, 1, 1), max_dist=0.01, iters=3)
    assert info["status"] == 2 and info["iterations"] == 1 and torch.equal(G4.cpu(), torch.eye(4, dtype=torch.float64).repeat(3, 1, 1))


def test_guards():
    points, normals, _ = SC.view_case(3)
    pts, idx = _scene(points, normals, 0.1)
    eye = torch.eye(4).repeat(5, 1, 1)
    with pytest.raises(ValueError, match="blocks"):
        scene_icp.refine_poses(pts[:1], idx[:1], eye[:1])
    with pytest.raises(ValueError, match="blocks"):
        scene_icp.refine_poses((pts * 2)[:5], (idx * 2)[:5], eye)
    with pytest.raises(ValueError, match="narrower"):
        scene_icp.refine_poses(pts, idx, eye[:3], max_dist=0.11)
    with pytest.raises(ValueError, match="N >= 1"):
        scene_icp.refine_poses([pts[0], pts[1][:0]], idx[:2], eye[:2], max_dist=0.1)
    # the library refuses each as well, before any launch
    lib = L.load()

    def blocks(K, empty=None):
        arr = (L.IcpBlock * K)()
        for b in range(K):
            ix = idx[b % 3]
            arr[b].src, arr[b].n = L.ptr(pts[b % 3]), (0 if b == empty else ix.n)
            arr[b].tgt_points, arr[b].tgt_normals, arr[b].cell_start = L.ptr(ix.points), L.ptr(ix.normals), L.ptr(ix.cell_start)
            arr[b].grid_lo, arr[b].cell = (L.c_float * 3)(*ix.lo), ix.cell
            arr[b].nx, arr[b].ny, arr[b].nz = ix.dims
        return arr
    nbytes = lib.dreg_icp_scene_workspace_bytes(3, blocks(3), None)
    assert nbytes > 0 and lib.dreg_icp_scene_workspace_bytes(1, blocks(1), None) == 0 and lib.dreg_icp_scene_workspace_bytes(5, blocks(5), None) == 0
    assert lib.dreg_icp_scene_workspace_bytes(3, blocks(3, empty=1), None) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    poses, st = _dev(np.tile(SC.identity_poses(1), (5, 1)), torch.float64), torch.zeros(1, 7, dtype=torch.float64, device=DEV)
    call = lambda K, blk, md, nb: lib.dreg_icp_scene_refine(K, blk, None, L.ptr(poses), md, 1, 1e-7, 1e-7, 1e-6, L.ptr(st), None, None, L.ptr(ws), nb, L.stream())
    assert call(1, blocks(1), 0.05, nbytes) == -1 and call(5, blocks(5), 0.05, nbytes) == -1
    assert call(3, blocks(3, empty=2), 0.05, nbytes) == -1
    assert call(3, blocks(3), 0.2, nbytes) == -1                       # cell < max_dist
    assert call(3, blocks(3), 0.05, nbytes - 8) == -1                  # workspace too small
    torch.cuda.synchronize()
    assert not st.any().item()                                          # nothing was launched
    assert call(3, blocks(3), 0.05, nbytes) == 0
    torch.cuda.synchronize()
    assert st[0, 0].item() > 0


def test_evaluator_refine_scene_end_to_end(tmp_path, monkeypatch):
    """eval_nerf_regtr.py --synthetic 2 --synthetic_blocks 3 with --register_scene and with --refine_scene (untrained weights: plumbing; no
    accuracy claim on synthetic shells): scene_refined_metrics_test.json with its schema, scene_metrics_test.json byte-identical."""
    import importlib
    import random
    import sys

    def main(argv):
        monkeypatch.setattr(sys, "argv", ["eval_nerf_regtr.py"] + argv)
        monkeypatch.syspath_prepend(ROOT)
        state = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
        try:
            importlib.import_module("eval_nerf_regtr").main()
        finally:
            random.setstate(state[0])
            np.random.set_state(state[1])
            torch.set_rng_state(state[2])
            torch.cuda.set_rng_state(state[3], DEV)
    common = ["--root_dir", str(tmp_path), "--synthetic", "2", "--synthetic_res", "32", "--precision", "fp32", "--synthetic_blocks", "3"]
    main(common + ["--expname", "scene", "--register_scene"])
    main(common + ["--expname", "refined", "--refine_scene"])
    base = lambda name: os.path.join(str(tmp_path), "eval", name, "synthetic")
    assert sorted(os.listdir(base("scene"))) == ["metrics_test.json", "scene_metrics_test.json"]
    assert sorted(os.listdir(base("refined"))) == ["metrics_test.json", "scene_metrics_test.json", "scene_refined_metrics_test.json"]
    read = lambda name, f: open(os.path.join(base(name), f), "rb").read()
    assert read("scene", "scene_metrics_test.json") == read("refined", "scene_metrics_test.json")
    sync = json.loads(read("refined", "scene_metrics_test.json"))
    js = json.loads(read("refined", "scene_refined_metrics_test.json"))
    assert set(js) == set(sync) | {"R_mean_sync", "t_mean_sync"}
    for s in ("shell_0000", "shell_0001"):
        assert set(js[s]) == set(sync[s]) | {"status", "iterations", "fitness", "R_mean_sync", "t_mean_sync"}
        assert js[s]["status"] in (0, 1, 2, 3) and 1 <= js[s]["iterations"] <= 30 and 0.0 <= js[s]["fitness"] <= 1.0
        assert js[s]["R_mean_sync"] == sync[s]["R_mean"] and len(js[s]["blocks"]) == 3 and len(js[s]["edges"]) == 6
        if js[s]["status"] in (2, 3):
            assert {k: js[s][k] for k in sync[s]} == sync[s]
