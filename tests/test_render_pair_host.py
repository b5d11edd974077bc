"""CPU: the host side of the two-block renderer.  render.rays_to_block by hand; the CPU restatement of the merged-stream rule
(tests/render_pair_restatement.py) against closed forms — disjoint slabs, coincident slabs and the overlap weight, the tie order, weight_src;
and the flag, files and merged_metrics.json of eval_nerf_regtr.py --render_merged with a stub renderer."""
import json
import math

import numpy as np
import pytest
import torch
from PIL import Image

import render_pair_restatement as RP
from dreg_nerf_amd import render as R
from dreg_nerf_amd.config import config_parser


# ------------------------------------------------------------------------------------------------------- the ray transform
def _pose(angle_deg, axis, t):
    a = math.radians(angle_deg)
    c, s = math.cos(a), math.sin(a)
    Rm = {"z": [[c, -s, 0], [s, c, 0], [0, 0, 1]], "x": [[1, 0, 0], [0, c, -s], [0, s, c]]}[axis]
    P = torch.eye(4, dtype=torch.float64)
    P[:3, :3] = torch.tensor(Rm, dtype=torch.float64)
    P[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return P


def test_rays_to_block_by_hand_90_degrees():
    P = torch.tensor([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]])          # [3,4]: x -> y, y -> -x, then t = (1, 2, 3)
    rays = R.Rays(torch.tensor([[1.0, 3.0, 3.0], [1.0, 2.0, 3.0]]), torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    got = R.rays_to_block(rays, P)
    # o - t = (0, 1, 0) and (0, 0, 0); R^T maps y -> x
    assert torch.equal(got.origins, torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    assert torch.equal(got.viewdirs, torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]))
    # a point of the source frame lands where P puts it: P (o_S + s d_S) = o + s d
    x_s = got.origins[0] + 2.5 * got.viewdirs[0]
    assert torch.allclose(P[:, :3] @ x_s + P[:, 3], rays.origins[0] + 2.5 * rays.viewdirs[0])
    # the [4,4] form gives the same rays, and [H,W,3] shapes are kept
    P4 = torch.cat([P, torch.tensor([[0.0, 0.0, 0.0, 1.0]])])
    again = R.rays_to_block(R.Rays(rays.origins.view(1, 2, 3), rays.viewdirs.view(1, 2, 3)), P4)
    assert again.origins.shape == (1, 2, 3) and torch.equal(again.origins.view(2, 3), got.origins) and again.origins.dtype == torch.float32


def test_rays_to_block_round_trip_and_unit_directions():
    g = torch.Generator().manual_seed(1)
    P = _pose(25.0, "z", (0.3, -0.2, 0.1)) @ _pose(-40.0, "x", (0.0, 0.0, 0.0))
    o = torch.randn(500, 3, generator=g) * 2
    d = torch.nn.functional.normalize(torch.randn(500, 3, generator=g), dim=-1)
    there = R.rays_to_block(R.Rays(o, d), P)
    back = R.rays_to_block(there, torch.linalg.inv(P))
    assert (back.origins - o).abs().max().item() <= 1e-6 * max(1.0, o.abs().max().item()) and (back.viewdirs - d).abs().max().item() <= 1e-6
    # unit to one ulp of 1: each fp32 component is within 2^-24 relative of a unit fp64 vector
    assert (there.viewdirs.double().norm(dim=-1) - 1.0).abs().max().item() <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------------- the restatement vs closed forms
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]


def _slab(z_cells):
    b = torch.zeros(8, 8, 8, dtype=torch.bool)                      # cells of 0.25 over [-1, 1]
    b[:, :, z_cells] = True
    return b


def _const_field(sigma, rgb):
    return lambda x, d: (torch.full((x.shape[0],), float(sigma)), torch.tensor(rgb).expand(x.shape[0], 3))


def _block(field, binary, dt, center=(0.0, 0.0, -3.0), **kw):
    return dict(field=field, binary=binary, roi_aabb=AABB, scene_aabb=AABB, dt=dt, center=center, **kw)


def _z_rays():
    o = torch.tensor([[-0.3, 0.1, -3.0], [0.2, -0.5, -3.0], [0.0, 0.0, -3.0]])
    d = torch.tensor([[0.0, 0.0, 1.0]]).expand(3, 3).contiguous()
    return o, d


RED, GREEN = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)


def test_disjoint_slabs_front_over_back():
    """S fills z in [-1, -0.5), T fills z in [0, 0.5); identity pose, each block on its own step."""
    sig_s, sig_t, L = 1.5, 0.8, 0.5
    src = _block(_const_field(sig_s, RED), _slab(slice(0, 2)), 0.1)
    tgt = _block(_const_field(sig_t, GREEN), _slab(slice(4, 6)), 0.05)
    rays = _z_rays()
    out = RP.render_pair(src, tgt, rays, rays, bkgd=(1.0, 1.0, 1.0))
    e_s, e_t = math.exp(-sig_s * L), math.exp(-sig_t * L)
    tol = max(sig_s * src["dt"], sig_t * tgt["dt"])                  # the lattice error of a slab's optical depth
    assert (out["omega"] == 1).all()
    assert (out["opacity"] - (1 - e_s * e_t)).abs().max().item() <= tol
    want = torch.tensor(RED) * (1 - e_s) + e_s * (1 - e_t) * torch.tensor(GREEN) + e_s * e_t * torch.ones(3)
    assert (out["rgb"] - want).abs().max().item() <= tol
    assert (out["weight_src"] - (1 - e_s)).abs().max().item() <= tol
    assert out["n_samples"] == 3 * (5 + 10)
    # the back block in front instead: swap the slabs' roles and the colours swap places in the composite
    out2 = RP.render_pair(_block(_const_field(sig_s, RED), _slab(slice(4, 6)), 0.1), _block(_const_field(sig_t, GREEN), _slab(slice(0, 2)), 0.05), rays, rays)
    want2 = torch.tensor(GREEN) * (1 - e_t) + e_t * (1 - e_s) * torch.tensor(RED)
    assert (out2["rgb"] - want2).abs().max().item() <= tol and (out2["weight_src"] - e_t * (1 - e_s)).abs().max().item() <= tol


def test_coincident_slabs_are_not_counted_twice():
    """Both blocks model the same slab z in [-0.5, 0.5) and their cameras share a centroid: omega = 1/2 each, the pair renders the single slab."""
    sigma, L, dt = 1.0, 1.0, 0.05
    mk = lambda: _block(_const_field(sigma, RED), _slab(slice(2, 6)), dt)
    rays = _z_rays()
    out = RP.render_pair(mk(), mk(), rays, rays)
    marched = out["alpha"] > 0
    assert marched.any() and (out["omega"][marched] == 0.5).all()
    single, double = 1 - math.exp(-sigma * L), 1 - math.exp(-2 * sigma * L)
    tol = sigma * dt
    assert (out["opacity"] - single).abs().max().item() <= tol
    assert (out["weight_src"] - 0.5 * single).abs().max().item() <= tol
    # without the weight the shared region counts twice, and the bound tells the two apart
    naive = RP.render_pair(mk(), mk(), rays, rays, use_omega=False)
    assert (naive["opacity"] - double).abs().max().item() <= tol and double - single > 2 * tol
    # a nearer source centroid moves the weight towards the source: omega_S = 1 / (1 + q^(p/2)) with q = (|x - c_S| / |x - c_T|)^2
    near = RP.render_pair(_block(_const_field(sigma, RED), _slab(slice(2, 6)), dt, center=(0.0, 0.0, -1.0)), mk(), (rays[0][2:], rays[1][2:]),
                          (rays[0][2:], rays[1][2:]), power=2.0)
    k = int(torch.nonzero(near["is_src"][0] & (near["alpha"][0] > 0))[0])
    z = -3.0 + float(near["t"][0, k])
    q = ((z + 1.0) / (z + 3.0)) ** 2
    assert abs(float(near["omega"][0, k]) - 1 / (1 + q)) <= 1e-6 and float(near["omega"][0, k]) > 0.5
    assert abs(float(near["omega"][0, k]) + float(near["omega"][0, k + 1]) - 1.0) <= 1e-6         # the target's sample at the same t


def test_tie_order_source_first():
    """Equal lattices and two opaque blocks: every t_mid is a tie, and the source's sample is composited first."""
    dt = 0.1
    rays = _z_rays()
    out = RP.render_pair(_block(_const_field(1e3, RED), _slab(slice(2, 6)), dt), _block(_const_field(1e3, GREEN), _slab(slice(2, 6)), dt), rays, rays)
    assert torch.equal(out["t"][:, 0], out["t"][:, 1]) and out["is_src"][:, 0].all() and not out["is_src"][:, 1].any()
    assert (out["rgb"] - torch.tensor(RED)).abs().max().item() <= 1e-6 and (out["weight_src"] - out["opacity"]).abs().max().item() <= 1e-6
    swapped = RP.render_pair(_block(_const_field(1e3, GREEN), _slab(slice(2, 6)), dt), _block(_const_field(1e3, RED), _slab(slice(2, 6)), dt), rays, rays)
    assert (swapped["rgb"] - torch.tensor(GREEN)).abs().max().item() <= 1e-6


def test_weight_src_with_one_block_empty():
    import render_restatement as RR
    dt = 0.1
    rays = _z_rays()
    full, empty = _block(_const_field(0.7, RED), _slab(slice(2, 6)), dt), _block(_const_field(0.7, GREEN), torch.zeros(8, 8, 8, dtype=torch.bool), dt)
    one = RR.render(full["field"], rays[0], rays[1], full["binary"], AABB, AABB, dt, bkgd=(1.0, 1.0, 1.0))
    a = RP.render_pair(empty, full, rays, rays, bkgd=(1.0, 1.0, 1.0))
    assert torch.equal(a["weight_src"], torch.zeros(3)) and a["n_samples"] == one[3]
    close = lambda x, y: (x - y).abs().max().item() <= 1e-6          # (the same samples summed over a longer, merged list)
    assert close(a["rgb"], one[0]) and close(a["opacity"], one[1]) and close(a["depth"], one[2])
    b = RP.render_pair(full, empty, rays, rays, bkgd=(1.0, 1.0, 1.0))
    assert torch.equal(b["weight_src"], b["opacity"]) and close(b["opacity"], one[1]) and close(b["rgb"], one[0])
    # both empty, or a ray that misses both: the background, 0, 0, 0
    c = RP.render_pair(empty, empty, rays, rays, bkgd=(0.25, 0.5, 1.0))
    assert c["n_samples"] == 0 and torch.equal(c["rgb"], torch.tensor([0.25, 0.5, 1.0]).expand(3, 3)) and not c["opacity"].any() and not c["depth"].any()


# ------------------------------------------------------------------------------------------------------- --render_merged: flag, files, json
def test_render_merged_flag_parses():
    assert config_parser([]).render_merged is False
    cfg = config_parser(["--render_merged"])
    assert cfg.render_merged is True and cfg.render_views is False


def test_render_merged_files_and_metrics_schema(tmp_path, monkeypatch):
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

    def stub(pose, poses, K, W_, H_):
        assert (W_, H_) == (W, H) and torch.equal(K, R.intrinsics("objaverse")[0])
        seen.append((pose.clone(), poses.clone()))
        n = poses.shape[0]
        level = 0.25 * len(seen)
        return ([torch.full((H, W, 3), level) for _ in range(n)], [torch.linspace(0, 1, H * W).reshape(H, W, 1) for _ in range(n)],
                [torch.full((H, W, 1), 1.0 if i % 2 else 0.0) for i in range(n)])

    def metrics(pred, gt):
        assert len(pred) == len(gt) == 5 and float(pred[0][0, 0, 0]) == 0.5 and float(gt[0][0, 0, 0]) == 0.25      # aligned against gt
        return [20.0 + i for i in range(5)], [0.5 + 0.1 * i for i in range(5)]

    out = tmp_path / "scene"
    res = R.render_scene_merged(str(out), src_p, tgt_p, P_gt, P_pred, "objaverse", "cpu", renderer=stub, metrics=metrics)
    # two sets; every camera of both blocks in the TARGET frame: (P @ src cameras, tgt cameras)
    assert len(seen) == 2 and torch.equal(seen[0][0], P_gt) and torch.equal(seen[1][0], P_pred)
    assert torch.allclose(seen[0][1], torch.cat([P_gt @ src_c, tgt_c]), atol=1e-6) and torch.allclose(seen[1][1], torch.cat([P_pred4 @ src_c, tgt_c]), atol=1e-6)
    for prefix in ("gt", "aligned"):
        d = out / f"{prefix}_merged_images"
        assert sorted(p.name for p in d.iterdir()) == sorted(f"{kind}_{i}.png" for kind in ("rgb", "depth", "src_share") for i in range(5))
        for p in d.iterdir():
            im = Image.open(p)
            assert im.size == (W, H) and im.mode == "RGB", p
        share = np.asarray(Image.open(d / "src_share_1.png"))
        assert (share == 255).all() and (np.asarray(Image.open(d / "src_share_0.png")) == 0).all()          # weight_src as a grey image
    assert not (out / "unaligned_merged_images").exists()
    assert (np.asarray(Image.open(out / "gt_merged_images" / "rgb_0.png")) == 63).all() and (np.asarray(Image.open(out / "aligned_merged_images" / "rgb_0.png")) == 127).all()
    js = json.loads((out / "merged_metrics.json").read_text())
    assert js == res and set(js) == {"views", "psnr_mean", "ssim_mean"}
    assert len(js["views"]) == 5 and all(set(v) == {"psnr", "ssim"} for v in js["views"])
    assert js["views"][3] == {"psnr": 23.0, "ssim": pytest.approx(0.8)} and js["psnr_mean"] == pytest.approx(22.0) and js["ssim_mean"] == pytest.approx(0.7)
