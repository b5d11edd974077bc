"""CPU: the differentiable-pose fixtures (tools/make_golden_pose_grad.py, from the reference's own autograd) against the oracle, and the
boundary of the feature: the two backward symbols in the header and the binding, the command-line flags of the pose loss."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import regtr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WELL_POSED = ["n3", "n17", "n255", "n256", "n257", "n3000", "zeros", "reflection", "small_sum"]


@pytest.mark.parametrize("case", WELL_POSED)
def test_kabsch_fixture_equals_oracle_autograd(golden_dir, case):
    z = np.load(os.path.join(golden_dir, "kabsch_grad.npz"))
    a, b, w = (torch.from_numpy(z[f"{case}/{k}"]).double().requires_grad_(True) for k in ("a", "b", "w"))
    g = torch.from_numpy(z[f"{case}/g_out"]).double()
    T = O.weighted_kabsch(a, b, w)
    np.testing.assert_allclose(T.detach().numpy(), z[f"{case}/pose"], atol=1e-10)
    (T * g).sum().backward()
    for t, k in ((a, "g_a"), (b, "g_b"), (w, "g_w")):
        ref = z[f"{case}/{k}"]
        assert np.linalg.norm(t.grad.numpy() - ref) <= 1e-8 * np.linalg.norm(ref), (case, k)


def test_kabsch_fixture_covers_the_branches(golden_dir):
    z = np.load(os.path.join(golden_dir, "kabsch_grad.npz"))
    cases = {k.split("/")[0] for k in z.files}
    assert {"n3", "n17", "n255", "n256", "n257", "n3000", "zeros", "reflection", "small_sum", "planar"} <= cases
    assert (z["zeros/w"] == 0).any()
    assert z["small_sum/w"].sum() < 1e-6                                     # the clamp of the weight sum (eps = 1e-6)
    a, b = z["reflection/a"].astype(np.float64), z["reflection/b"].astype(np.float64)
    w = z["reflection/w"].astype(np.float64)[:, None] / z["reflection/w"].sum()
    H = ((a - (w * a).sum(0)) * w).T @ (b - (w * b).sum(0))
    u, _, vt = np.linalg.svd(H)
    assert np.linalg.det(vt.T @ u.T) < 0                                     # d = -1: the reference flips V
    s = np.linalg.svd(np.cov(z["planar/a"].T), compute_uv=False)
    assert s[2] < 1e-5 * s[0]
    for k in z.files:
        assert np.isfinite(z[k]).all(), k


def test_pose_grad32_fixture_fp32_close_to_fp64(golden_dir):
    g = np.load(os.path.join(golden_dir, "pose_grad32.npz"))
    assert np.isfinite(float(g["loss"])) and abs(float(g["loss"]) - float(g["loss64"])) <= 1e-5 * float(g["loss64"])
    for name in ("transformer", "decoder"):
        np.testing.assert_allclose(float(g["gnorm_" + name]), float(g["gnorm64_" + name]), rtol=1e-3)
    assert g["pose"].shape[0] == 6


def test_backward_symbols_declared_and_bound():
    from dreg_nerf_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dreg_nerf.h")).read(), flags=re.S)
    for name in ("dreg_weighted_kabsch_bwd", "dreg_weighted_kabsch_pairs_bwd"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in lib.declared_symbols()


def test_pose_loss_flags():
    from dreg_nerf_amd.config import config_parser
    cfg = config_parser([])
    assert cfg.pose_loss_weight == 0.0 and cfg.pose_loss_layers == "last"
    cfg = config_parser(["--pose_loss_weight", "0.3", "--pose_loss_layers", "all"])
    assert cfg.pose_loss_weight == 0.3 and cfg.pose_loss_layers == "all"
    src = open(os.path.join(ROOT, "train_nerf_regtr.py")).read()
    assert "pose_loss_weight=cfg.pose_loss_weight" in src and "pose_loss_layers=cfg.pose_loss_layers" in src
