"""CPU: the joint K-block ICP rule in its fp64 restatement (tests/scene_icp_restatement.py) — the assembled gradient and
Gauss-Newton matrix against central differences, K = 2 against the pair rule, planted assembly errors, convergence on three partial views of
the test solid, the failure statuses — and the files, schema and fallbacks of eval_nerf_regtr.py --refine_scene with injected stubs."""
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import icp_cases as IC
import icp_restatement as IR
import scene_icp_cases as SC
import scene_icp_restatement as SR
from dreg_nerf_amd import dataset as D
from dreg_nerf_amd import scene_icp, scene_reg  # noqa: F401  (scene_icp: the module under test must exist)
from dreg_nerf_amd.config import config_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ derivatives
H_G, H_H = 1e-5, 1e-4              # steps of the central differences for the gradient and for the second derivatives


def _fixed(K, at_truth):
    """(points, normals, G12, corrs, N): fp64 clouds, the correspondences fixed at G12 = the true poses (every residual ~1e-16: the Gauss-Newton
    matrix is then the whole Hessian) or at the identity (residuals of the size of the motions: a gradient worth the name)."""
    pts, nrm, G_true = SC.view_case(K, fp32=False)
    G12 = G_true if at_truth else SC.identity_poses(K)
    cids = SR.cell_ids([p.astype(np.float32) for p in pts], IC.MAX_DIST)
    corrs = SR.pair_correspondences(pts, nrm, cids, SR.rel_poses(G12), IC.MAX_DIST)
    return pts, nrm, G12, corrs, sum(int((c >= 0).sum()) for c in corrs.values())


def _moved(G12, steps):
    out = G12.copy()
    for k, h in steps:
        x = np.zeros(6)
        x[k % 6] = h
        out[k // 6] = SR.perturbed(out[k // 6], x)
    return out


def _tolerances(N, f0):
    """Along a unit direction every residual is e(s) = e0 + J s + c s^2 / 2 + d s^3 / 6 + ..., with the points within |x| <= 2 of the origin:
    |J| <= sqrt(|x|^2 + 1) <= 2.3, and each further derivative gains at most a factor |x| + 1 <= 3 (one more cross product with a unit axis, for
    either end of the pair): |c| <= 7, |d| <= 21.  For f = sum e^2 over N residuals with |e0| <= 0.1 (the gate):
    f''' = sum (6 J c + 2 e0 d) <= 101 N, the central first difference errs by h^2 f''' / 6; with e0 = 0, f'''' = sum (6 c^2 + 8 J d) <= 681 N, the
    central second difference errs by h^2 f'''' / 12 and a mixed one (a sum of two such along the diagonals) by twice that.  Rounding: 2^-52 f0 / h
    and 4 * 2^-52 * max f / h^2 with max f <= N (2.3 h sqrt 2)^2."""
    tol_g = H_G ** 2 * 101.0 * N / 6.0 + 2.0 ** -52 * max(f0, 1.0) / H_G
    tol_h = 2.0 * H_H ** 2 * 681.0 * N / 12.0 + 4.0 * 2.0 ** -52 * N * 10.6
    return tol_g, tol_h


def _derivative_errors(K, variant=None):
    """(|2 g - central differences|_max, its tolerance, |2 H - central differences|_max, its tolerance)."""
    out = []
    for at_truth in (False, True):
        pts, nrm, G12, corrs, N = _fixed(K, at_truth)
        rel = SR.rel_poses(G12)
        S = SR.pair_sums(pts, nrm, corrs, rel, round_pose=False)
        H, g, _ = SR.assemble(S, G12, SR.enabled_pairs(K), variant)
        f = lambda steps: SR.cost(pts, nrm, corrs, _moved(G12, steps))
        tol_g, tol_h = _tolerances(N, f([]))
        n = 6 * K
        if not at_truth:
            fd = np.array([(f([(k, H_G)]) - f([(k, -H_G)])) / (2 * H_G) for k in range(n)])
            out += [float(np.abs(2 * g - fd).max()), tol_g, float(np.abs(2 * g).max())]
        else:
            f0 = f([])
            fd = np.zeros((n, n))
            for a in range(n):
                fd[a, a] = (f([(a, H_H)]) - 2 * f0 + f([(a, -H_H)])) / H_H ** 2
                for b in range(a + 1, n):
                    fd[a, b] = fd[b, a] = (f([(a, H_H), (b, H_H)]) - f([(a, H_H), (b, -H_H)]) - f([(a, -H_H), (b, H_H)]) + f([(a, -H_H), (b, -H_H)])) / (4 * H_H ** 2)
            out += [float(np.abs(2 * H - fd).max()), tol_h, float(np.abs(2 * H).max())]
    return out


@pytest.mark.parametrize("K", [3, 4])
def test_gradient_and_gauss_newton_matrix_against_central_differences(K):
    eg, tg, mg, eh, th, mh = _derivative_errors(K)
    print(f"K {K}: |2g - fd| {eg:.3e} (tolerance {tg:.3e}, |2g|max {mg:.3e}); |2H - fd| {eh:.3e} (tolerance {th:.3e}, |2H|max {mh:.3e})")
    assert eg <= tg and eh <= th
    assert tg < 1e-4 * mg and th < 1e-4 * mh            # the tolerances are far below the quantities they test


@pytest.mark.parametrize("variant", ["sign", "adjoint", "lower_left", "swapped"])
def test_planted_assembly_errors_are_seen(variant):
    eg, tg, _, eh, th, _ = _derivative_errors(3, variant)
    factor = max(eg / tg, eh / th)
    print(f"{variant}: gradient error / tolerance {eg / tg:.3e}, matrix error / tolerance {eh / th:.3e}")
    assert factor > 100.0


# ------------------------------------------------------------------------------------------------------------------ K = 2 is the pair rule
def test_two_blocks_with_one_direction_equal_the_pair_refinement():
    """Only (1 -> 0) enabled and G_0 = I: rel[1][0] = G_1 and the adjoint is the identity, so the run is IR.refine on (block 1, block 0) up to the
    rounding of the two operation orders (M^T A' M with M = I adds exact zeros; rel = I^T G_1 is exact): the poses agree to 1e-12."""
    pts, nrm, G_true = SC.view_case(2)
    mask = np.array([[0, 0], [1, 0]], dtype=np.uint8)
    G, stats = SR.refine(pts, nrm, SC.identity_poses(2), IC.MAX_DIST, 4, cell=IC.MAX_DIST, pair_mask=mask)
    pose, pstats = IR.refine(pts[1], pts[0], nrm[0], SC.identity_poses(2)[1], IC.MAX_DIST, 4, cell=IC.MAX_DIST)
    print("largest pose difference", float(np.abs(G[1] - pose).max()), "stats difference", float(np.abs(stats - pstats).max()))
    assert np.array_equal(G[0], SC.identity_poses(2)[0])
    assert np.abs(G[1] - pose).max() <= 1e-12 and np.array_equal(stats[:, [0, 6]], pstats[:, [0, 6]])
    assert np.allclose(stats, pstats, rtol=1e-9, atol=1e-15)


# ------------------------------------------------------------------------------------------------------------------ convergence, statuses
def test_three_views_of_the_test_solid_converge():
    pts, nrm, G_true = SC.view_case(3)
    assert [len(p) for p in pts] == [971, 767, 1002]
    iters = IC.MAX_ITERS + 2
    G, stats = SR.refine(pts, nrm, SC.identity_poses(3), IC.MAX_DIST, iters, cell=IC.MAX_DIST)
    for k in range(iters):
        print(f"iteration {k + 1}: count {stats[k, 0]:.0f}, max |omega| {stats[k, 3]:.3e}, max |v| {stats[k, 4]:.3e}, status {stats[k, 6]:.0f}")
    rre, rte = SC.worst_errors(G, G_true)
    print(f"worst RRE {rre:.3e} deg, worst RTE {rte:.3e}")
    done = int(np.nonzero(stats[:, 6])[0][0]) + 1
    assert rre <= IC.RRE_BOUND_DEG and rte <= IC.RTE_BOUND
    assert stats[done - 1, 6] == 1 and done <= IC.MAX_ITERS and all(np.array_equal(stats[k], stats[done - 1]) for k in range(done, iters))
    assert np.array_equal(G[0], SC.identity_poses(3)[0])


def test_failure_statuses_leave_the_poses_untouched():
    pts, nrm, _ = SC.view_case(3)
    start = SC.identity_poses(3)
    far = [pts[0], pts[1], pts[2] + np.float32(10.0)]                 # block 2 beyond the gate of both others: its diagonal block is zero
    G, stats = SR.refine(far, nrm, start, IC.MAX_DIST, 2, cell=IC.MAX_DIST)
    assert np.array_equal(G, start) and np.all(stats[:, 6] == 3) and stats[0, 0] > 12
    few = [np.concatenate([pts[0][:3], pts[0][3:40] + np.float32(10.0)]), pts[0][:2], pts[0][:1]]      # 2 + 1 + 2 + 1 + 1 + 1 = 8 correspondences < 12
    fn = [nrm[0][:40], nrm[0][:2], nrm[0][:1]]
    G, stats = SR.refine(few, fn, start, 0.01, 2, cell=0.01)
    print("too few: count", stats[0, 0])
    assert np.array_equal(G, start) and np.all(stats[:, 6] == 2) and 0 < stats[0, 0] < 12


# ------------------------------------------------------------------------------------------------------------------ --refine_scene
def _evaluator():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("eval_nerf_regtr")


def _gt_pair_fn(i, j, sample):
    return sample["pose"][0].double()[:3]


def test_refine_scene_files_schema_fallback_and_products(tmp_path, monkeypatch):
    E = _evaluator()
    quiet = lambda *a, **k: None
    ds = D.SyntheticRegDataset(2, 8, "test", n_blocks=3)
    assert config_parser(["--refine_scene"]).refine_scene and E.implied_flags(config_parser(["--refine_scene"])).register_scene
    assert not config_parser([]).refine_scene

    def run(flags, sub, refiner=None):
        cfg = E.implied_flags(config_parser(flags + ["--root_dir", str(tmp_path / sub), "--expname", "t", "--dataset", ""]))
        d = tmp_path / sub / "eval" / "t" / "synthetic"
        refined = {}
        rows = E.register_scenes(cfg, ds, None, "cpu", pair_fn=_gt_pair_fn, log=quiet, refiner=refiner, refined_rows=refined)
        E.write_scenes(str(d), "test", rows, log=quiet)
        if refined:
            E.write_scenes_refined(str(d), "test", refined, log=quiet)
        return d, rows, refined

    calls = []

    def refiner(scene, G_sync):
        """Scene 0: a refinement that moves block 1 by 2 degrees; scene 1: a degenerate run (status 3) whose poses must not be used."""
        calls.append(len(scene))
        G = torch.as_tensor(G_sync).double().clone()
        Rz = torch.tensor(SR.poses44_of([IR.pose12_of(IC.rotation((0, 0, 1), 2.0), np.zeros(3))])[0])
        G[1] = Rz @ G[1]
        status = 0 if len(calls) == 1 else 3
        return G, {"status": status, "iterations": 4, "fitness": 0.5, "plane_rmse": 0.0, "inlier_rmse": 0.0}

    d0, rows0, none = run(["--register_scene"], "plain")
    d1, rows1, refined = run(["--refine_scene"], "refined", refiner)
    assert none == {} and calls == [3, 3]
    assert sorted(os.listdir(d0)) == ["scene_metrics_test.json"] and sorted(os.listdir(d1)) == ["scene_metrics_test.json", "scene_refined_metrics_test.json"]
    assert (d0 / "scene_metrics_test.json").read_bytes() == (d1 / "scene_metrics_test.json").read_bytes()
    js = json.loads((d1 / "scene_refined_metrics_test.json").read_text())
    base = json.loads((d1 / "scene_metrics_test.json").read_text())
    assert set(js) == set(base) | {"R_mean_sync", "t_mean_sync"}
    extra = {"status", "iterations", "fitness", "R_mean_sync", "t_mean_sync"}
    for name in ("shell_0000", "shell_0001"):
        assert set(js[name]) == set(base[name]) | extra
        assert js[name]["R_mean_sync"] == base[name]["R_mean"] and js[name]["t_mean_sync"] == base[name]["t_mean"]
        assert js[name]["iterations"] == 4 and js[name]["fitness"] == 0.5
    a, b = js["shell_0000"], js["shell_0001"]
    assert a["status"] == 0 and a["blocks"][1]["rre"] == pytest.approx(2.0, abs=1e-3) and a["blocks"][2]["rre"] < 0.1 and a["R_mean"] == pytest.approx(1.0, abs=0.05)   # (the metric is fp32)
    assert b["status"] == 3 and {k: b[k] for k in base["shell_0001"]} == base["shell_0001"]           # status 3: the synchronised poses, row for row
    assert js["R_mean"] == pytest.approx((a["R_mean"] + b["R_mean"]) / 2) and js["R_mean_sync"] == base["R_mean"]

    # the scene products take the refined poses, or the synchronised ones after status 2 / 3
    seen = []
    monkeypatch.setattr(scene_reg, "render_registered_scene", lambda out, scene, G_gt, G, *a, **k: seen.append(torch.as_tensor(G).clone()) or {"psnr_mean": 0.0, "ssim_mean": 0.0})
    calls.clear()
    cfg = E.implied_flags(config_parser(["--refine_scene", "--render_scene", "--root_dir", str(tmp_path / "r"), "--expname", "t", "--dataset", ""]))
    lines = []
    E.register_scenes(cfg, ds, None, "cpu", pair_fn=_gt_pair_fn, renderer=lambda *a: None, log=lambda m, **k: lines.append(m), refiner=refiner, refined_rows={})
    G_gt = [scene_reg.ground_truth(ds.get_scene(i)) for i in range(2)]
    assert len(seen) == 2 and IR.rre_deg(seen[0][1, :3, :3].numpy(), G_gt[0][1, :3, :3].numpy()) == pytest.approx(2.0, abs=1e-3)
    assert IR.rre_deg(seen[1][1, :3, :3].numpy(), G_gt[1][1, :3, :3].numpy()) < 1e-3
    assert any("refined poses" in m for m in lines) and any("synchronised poses (the refinement ended" in m for m in lines)
