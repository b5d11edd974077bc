"""CPU: the host side of the volume renderer (dreg_nerf_amd/render.py): pixel rays and intrinsics, the CPU restatement of the marching /
compositing rule (tests/render_restatement.py) against closed forms, and the files and pose sets of eval_nerf_regtr.py --render_views with a stub
renderer."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import render_restatement as RR
from dreg_nerf_amd import render as R


def test_pixel_rays_by_hand():
    K = torch.tensor([[2.0, 0, 1.5], [0, 4.0, 1.5], [0, 0, 1]])
    c2w = torch.eye(4)
    rays = R.pixel_rays(c2w, K, 3, 3)
    assert rays.origins.shape == (3, 3, 3) and rays.viewdirs.shape == (3, 3, 3)
    # the centre pixel looks down -z (OpenGL): ((1 - 1.5 + 0.5) / 2, -(1 - 1.5 + 0.5) / 4, -1)
    assert torch.equal(rays.viewdirs[1, 1], torch.tensor([0.0, 0.0, -1.0]))
    # pixel (x=2, y=0): (1 / 2, -(-1) / 4, -1), normalised
    v = torch.tensor([0.5, 0.25, -1.0])
    assert torch.allclose(rays.viewdirs[0, 2], v / v.norm(), atol=1e-7)
    # OpenCV convention: y and z keep their sign
    cv = R.pixel_rays(c2w, K, 3, 3, opengl=False)
    v = torch.tensor([0.5, -0.25, 1.0])
    assert torch.allclose(cv.viewdirs[0, 2], v / v.norm(), atol=1e-7)
    # a rotated, translated camera: origin = translation, direction = R @ camera direction
    ang = 0.3
    Rz = torch.tensor([[math.cos(ang), -math.sin(ang), 0], [math.sin(ang), math.cos(ang), 0], [0, 0, 1.0]])
    Rx = torch.tensor([[1.0, 0, 0], [0, math.cos(1.1), -math.sin(1.1)], [0, math.sin(1.1), math.cos(1.1)]])
    c2w = torch.eye(4)
    c2w[:3, :3] = Rz @ Rx
    c2w[:3, 3] = torch.tensor([0.5, -2.0, 3.0])
    rays = R.pixel_rays(c2w, K, 3, 3)
    assert torch.allclose(rays.origins, c2w[:3, 3].expand(3, 3, 3))
    v = c2w[:3, :3] @ torch.tensor([0.5, 0.25, -1.0])
    assert torch.allclose(rays.viewdirs[0, 2], v / v.norm(), atol=1e-6)
    assert torch.allclose(rays.viewdirs.norm(dim=-1), torch.ones(3, 3), atol=1e-6)


def test_intrinsics_table():
    K, W, H = R.intrinsics("scannerf")
    assert (W, H) == (1440, 1080)
    assert torch.allclose(K, torch.tensor([[1522.1201085541113, 0, 727.9348613007779], [0, 1521.954743529035, 541.5426465751151], [0, 0, 1]]))
    for name in ("objaverse", "nerf_synthetic"):
        K, W, H = R.intrinsics(name)
        fx = 0.5 * 800 / np.tan(0.5 * 0.6911112070083618)
        assert (W, H) == (800, 800) and abs(float(K[0, 0]) - fx) < 1e-3 and float(K[1, 1]) == float(K[0, 0]) and float(K[0, 2]) == 400.0
    with pytest.raises(NotImplementedError):
        R.intrinsics("llff")


# ------------------------------------------------------------------------------------------------------- the restatement vs closed forms
AABB = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
FULL = torch.ones(8, 8, 8, dtype=torch.bool)


def _const_field(sigma, rgb=(0.2, 0.4, 0.6)):
    return lambda x, d: (torch.full((x.shape[0],), float(sigma)), torch.tensor(rgb).expand(x.shape[0], 3))


def _z_rays(n=3):
    o = torch.tensor([[-0.3, 0.1, -3.0], [0.2, -0.5, -3.0], [0.0, 0.0, -3.0]])[:n]
    d = torch.tensor([[0.0, 0.0, 1.0]]).expand(n, 3).contiguous()
    return o, d


def test_constant_sigma_slab_closed_form():
    dt, sigma = 0.1, 0.7
    o, d = _z_rays()
    rgb, opac, depth, ns, surv, _ = RR.render(_const_field(sigma), o, d, FULL, AABB, AABB, dt, bkgd=(1.0, 1.0, 1.0))
    # t in [2, 4): samples at 2.05, 2.15, ..., 3.95 — twenty of them, all occupied
    n = 20
    a = 1 - math.exp(-sigma * dt)
    assert ns == 3 * n and surv.sum(1).tolist() == [n] * 3
    assert torch.allclose(opac, torch.full((3,), 1 - math.exp(-sigma * dt) ** n), atol=1e-6)
    dep = sum(a * (1 - a) ** k * (2.0 + (k + 0.5) * dt) for k in range(n))
    assert torch.allclose(depth, torch.full((3,), dep), atol=1e-5)
    want = torch.tensor([0.2, 0.4, 0.6]) * opac[:, None] + (1 - opac[:, None])
    assert torch.allclose(rgb, want, atol=1e-6)
    # near / far planes clip the lattice: t in [2.5, 3.0) -> samples 2.55 .. 2.95
    _, opac2, _, ns2, _, _ = RR.render(_const_field(sigma), o, d, FULL, AABB, AABB, dt, near_plane=2.5, far_plane=3.0)
    assert ns2 == 3 * 5 and torch.allclose(opac2, torch.full((3,), 1 - math.exp(-sigma * dt) ** 5), atol=1e-6)
    # empty grid / a ray that misses: background only
    rgb3, opac3, depth3, ns3, _, _ = RR.render(_const_field(sigma), o, d, torch.zeros_like(FULL), AABB, AABB, dt, bkgd=(1.0, 0.5, 0.0))
    assert ns3 == 0 and torch.equal(opac3, torch.zeros(3)) and torch.equal(depth3, torch.zeros(3))
    assert torch.equal(rgb3, torch.tensor([1.0, 0.5, 0.0]).expand(3, 3))
    miss_o = torch.tensor([[5.0, 5.0, -3.0]])
    _, opac4, _, ns4, _, _ = RR.render(_const_field(sigma), miss_o, d[:1], FULL, AABB, AABB, dt)
    assert ns4 == 0 and float(opac4[0]) == 0.0


def test_alpha_thre_prunes_and_reweights_over_survivors():
    """alternating densities along z: with alpha_thre between the two alphas only the dense samples survive, and their weights use the
    transmittance over the survivors only (rendering() of the pruned list), while T_all runs over every marched sample."""
    dt = 0.1
    hi_s, lo_s = 2.0, 0.05

    def field(x, d):
        k = torch.floor((x[:, 2] + 1.0) / dt + 1e-4).long()          # lattice index along z
        s = torch.where(k % 2 == 0, torch.full_like(x[:, 0], hi_s), torch.full_like(x[:, 0], lo_s))
        return s, torch.tensor([1.0, 0.0, 0.0]).expand(x.shape[0], 3)

    o, d = _z_rays(1)
    a_hi, a_lo = 1 - math.exp(-hi_s * dt), 1 - math.exp(-lo_s * dt)
    thre = 0.5 * (a_hi + a_lo)
    _, opac, depth, ns, surv, alpha = RR.render(field, o, d, FULL, AABB, AABB, dt, alpha_thre=thre)
    assert ns == 10 and surv[0, 0:20:2].all() and not surv[0, 1::2].any()
    w = [a_hi * (1 - a_hi) ** k for k in range(10)]                 # survivors only: the sparse samples do not attenuate
    assert abs(float(opac[0]) - sum(w)) < 1e-6
    assert abs(float(depth[0]) - sum(w[k] * (2.0 + (2 * k + 0.5) * dt) for k in range(10))) < 1e-5
    # without the threshold every sample survives and the weights follow the full product
    _, opac0, _, ns0, _, _ = RR.render(field, o, d, FULL, AABB, AABB, dt)
    assert ns0 == 20 and abs(float(opac0[0]) - (1 - ((1 - a_hi) * (1 - a_lo)) ** 10)) < 1e-6


def test_transmittance_cut_ends_the_ray():
    dt, sigma = 0.1, 30.0                                           # alpha = 0.95 per sample
    o, d = _z_rays(1)
    _, opac, _, ns, surv, _ = RR.render(_const_field(sigma), o, d, FULL, AABB, AABB, dt)
    q = math.exp(-sigma * dt)
    k = next(k for k in range(100) if q ** k < 1e-4)               # the first sample whose exclusive T_all is below early_stop_eps
    assert ns == k and surv[0, :k].all() and not surv[0, k:].any()
    assert abs(float(opac[0]) - (1 - q ** k)) < 1e-6


# ------------------------------------------------------------------------------------------------------- --render_views files, stub renderer
def test_render_views_files_and_pose_sets(tmp_path, monkeypatch):
    W, H = 8, 6
    monkeypatch.setitem(R.INTRINSICS, "objaverse", (W, H, 7.0, 7.0, 4.0, 3.0))
    g = torch.Generator().manual_seed(0)

    def cams(n):
        c = torch.eye(4).repeat(n, 1, 1)
        c[:, :3, 3] = torch.randn(n, 3, generator=g)
        return c
    src_c, tgt_c = cams(2), cams(3)
    src_p, tgt_p = str(tmp_path / "src.pth"), str(tmp_path / "tgt.pth")
    torch.save({"camera_poses": src_c}, src_p)
    torch.save({"camera_poses": tgt_c}, tgt_p)
    P_gt = torch.eye(4)
    P_gt[:3, 3] = torch.tensor([0.1, 0.2, 0.3])
    P_pred = torch.tensor([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, -0.2]])      # [3,4], as the model returns it
    P_pred4 = torch.cat([P_pred, torch.tensor([[0.0, 0.0, 0.0, 1.0]])])
    seen = []

    def stub(path, poses, K, W_, H_):
        assert (W_, H_) == (W, H) and torch.equal(K, R.intrinsics("objaverse")[0])
        seen.append((path, poses.clone()))
        z = poses[:, 2, 3]
        return [np.full((H, W, 3), 0.5, np.float32) for _ in z], [np.linspace(0, 1, H * W, dtype=np.float32).reshape(H, W, 1) + float(t) for t in z]

    out = tmp_path / "scene"
    R.render_scene_views(str(out), src_p, tgt_p, P_gt, P_pred, "objaverse", "cpu", renderer=stub)
    # three sets, source block then target block each
    assert [p for p, _ in seen] == [src_p, tgt_p] * 3
    exp = {"gt": (torch.cat([src_c, torch.linalg.inv(P_gt) @ tgt_c]), torch.cat([P_gt @ src_c, tgt_c])),
           "aligned": (torch.cat([src_c, torch.linalg.inv(P_pred4) @ tgt_c]), torch.cat([P_pred4 @ src_c, tgt_c])),
           "unaligned": (torch.cat([src_c, tgt_c]), torch.cat([src_c, tgt_c]))}
    for i, prefix in enumerate(("gt", "aligned", "unaligned")):
        assert torch.allclose(seen[2 * i][1], exp[prefix][0], atol=1e-6) and torch.allclose(seen[2 * i + 1][1], exp[prefix][1], atol=1e-6)
        for k in range(5):
            for sub, size in ((f"{prefix}_src_images/rgb_{k}.png", (W, H)), (f"{prefix}_tgt_images/rgb_{k}.png", (W, H)),
                              (f"{prefix}_images/src_tgt_rgb_depth_{k}.png", (4 * W, H))):
                im = Image.open(out / sub)
                assert im.size == size and im.mode == "RGB", sub
        assert not (out / f"{prefix}_images" / "src_tgt_rgb_depth_5.png").exists()
    # the composite: src rgb | jet-coloured src depth | tgt rgb | tgt depth
    im = np.asarray(Image.open(out / "gt_images" / "src_tgt_rgb_depth_0.png"))
    assert (im[:, :W] == 127).all() and (im[:, 2 * W:3 * W] == 127).all()
    dcol = R.colorize_depth(np.linspace(0, 1, H * W, dtype=np.float32).reshape(H, W))
    assert np.abs(im[:, W:2 * W].astype(int) - (dcol * 255).astype(np.uint8).astype(int)).max() <= 1


def test_colorize_depth_matches_the_percentile_rule():
    x = np.arange(100, dtype=np.float32).reshape(10, 10)
    c = R.colorize_depth(x)
    from matplotlib import colormaps
    vmin, vmax = np.percentile(x, (1, 100))
    want = colormaps["jet"]((np.clip(x, vmin, vmax + 1e-6) - vmin) / (vmax + 1e-6 - vmin))[:, :, :3]
    assert c.shape == (10, 10, 3) and np.allclose(c, want)
