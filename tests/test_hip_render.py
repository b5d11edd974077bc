"""GPU: the fused volume renderer (csrc/render.hip, dreg_nerf_amd/render.py) against the CPU restatement of its rule (tests/render_restatement.py,
built on the oracle's networks), its exact cases (missed rays, empty grid), bit-identity between runs and launch widths, the render_image drop-in's
shapes, and eval_nerf_regtr.py --render_views.

Tolerance (fp16 networks on both sides, different summation orders and exp implementations): >= 99 % of the pixels within 2e-2 in rgb and opacity
and within 2e-2 relative in depth; the surviving-sample count within 1 %.  The rest are pixels where one sample sits at a decision edge — an
alpha within rounding of alpha_thre, a transmittance within rounding of the 1e-4 cut, a lattice point on a cell face — and the two sides keep
a different sample."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import render_restatement as RR
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import ngp
from dreg_nerf_amd import render as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
W, H = 64, 48
K = torch.tensor([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1]])


def _block(seed=3, res=32, shell=(0.55, 1.05)):
    """A generated block like tests/test_hip_chain_config5.py's _make_block (random hash grid and MLPs, a thick occupancy shell), on the device."""
    g = torch.Generator().manual_seed(seed)
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params[:3072] = torch.randn(3072, generator=g) * 1.0
        f.mlp_base.params[3072:] = torch.randn(f.mlp_base.params.numel() - 3072, generator=g)
        f.color_mlp.params.copy_(torch.randn(7168, generator=g) * 0.2)
    base, color = f.mlp_base.params.detach().clone(), f.color_mlp.params.detach().clone()
    c = (torch.arange(res, dtype=torch.float32) + 0.5) / res * 3 - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    rad = torch.stack([X, Y, Z], -1).norm(dim=-1)
    binary = (rad > shell[0]) & (rad < shell[1])
    occ = ngp.OccupancyGrid(AABB, res)
    occ._binary.copy_(binary)
    return f.to(DEV).eval(), occ, base, color


def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target, up = torch.tensor(eye), torch.tensor(target), torch.tensor(up)
    back = torch.nn.functional.normalize(eye - target, dim=0)          # OpenGL: the camera looks down its -z
    right = torch.nn.functional.normalize(torch.linalg.cross(up, back), dim=0)
    true_up = torch.linalg.cross(back, right)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, true_up, back, eye
    return c2w


CAMERAS = {
    "outside": _look_at((2.6, -1.9, 1.2), (0.0, 0.0, 0.0)),
    "inside": _look_at((0.2, 0.1, 0.3), (1.0, 0.5, -0.4)),
    "partly_missing": _look_at((2.8, 2.6, 0.4), (1.2, 1.2, 0.0)),
}


@pytest.fixture(scope="module")
def block():
    return _block()


def _compare(hip, ref, frac=0.99, tol=2e-2):
    rgb, opac, depth, ns = hip
    rgb_r, opac_r, depth_r, ns_r = ref[:4]
    rgb, opac, depth = rgb.reshape(-1, 3).cpu(), opac.reshape(-1).cpu(), depth.reshape(-1).cpu()
    ok_rgb = ((rgb - rgb_r).abs().max(dim=1).values <= tol).float().mean().item()
    ok_op = ((opac - opac_r).abs() <= tol).float().mean().item()
    ok_dep = ((depth - depth_r).abs() <= tol * (depth_r.abs() + 0.05)).float().mean().item()
    assert ok_rgb >= frac and ok_op >= frac and ok_dep >= frac, (ok_rgb, ok_op, ok_dep)
    assert abs(ns - ns_r) <= max(0.01 * ns_r, 2), (ns, ns_r)


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("opts", [dict(), dict(alpha_thre=1e-2), dict(near_plane=0.4, far_plane=3.2)], ids=["plain", "alpha_thre", "near_far"])
def test_render_matches_restatement(block, cam, opts):
    f, occ, base, color = block
    dt = 0.02
    rays = R.pixel_rays(CAMERAS[cam].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    hip = R.render_image(f, occ, rays, AABB, render_step_size=dt, render_bkgd=bk, **opts)
    ref = RR.render(("ngp", base, color, torch.tensor(AABB)), rays.origins.reshape(-1, 3).cpu(), rays.viewdirs.reshape(-1, 3).cpu(), occ.binary,
                    AABB, AABB, dt, bkgd=bk, **opts)
    assert ref[3] > 1000, "the view sees too little of the block to test anything"
    _compare(hip, ref)
    if cam == "partly_missing":
        o, dd = rays.origins.reshape(-1, 3).cpu(), rays.viewdirs.reshape(-1, 3).cpu()
        _, _, hit = RR.ray_interval(o, dd, torch.tensor(AABB), opts.get("near_plane"), opts.get("far_plane"))
        assert 0 < int(hit.sum()) < hit.numel()
        miss = ~hit
        # missed rays: exactly the background, 0, 0
        assert torch.equal(hip[0].reshape(-1, 3).cpu()[miss], bk.expand(int(miss.sum()), 3))
        assert torch.equal(hip[1].reshape(-1).cpu()[miss], torch.zeros(int(miss.sum())))
        assert torch.equal(hip[2].reshape(-1).cpu()[miss], torch.zeros(int(miss.sum())))


def test_empty_grid_renders_the_background(block):
    f, occ, _, _ = block
    empty = ngp.OccupancyGrid(AABB, 32)
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    bk = torch.tensor([0.25, 0.5, 1.0])
    rgb, opac, depth, ns = R.render_image(f, empty, rays, AABB, render_step_size=0.02, render_bkgd=bk)
    assert ns == 0
    assert torch.equal(rgb.cpu(), bk.expand(H, W, 3)) and not opac.any() and not depth.any()


def test_bit_identical_between_runs_and_launch_widths(block):
    f, occ, _, _ = block
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    kw = dict(render_step_size=0.02, render_bkgd=torch.ones(3))
    a = R.render_image(f, occ, rays, AABB, **kw)
    b = R.render_image(f, occ, rays, AABB, **kw)
    assert a[3] == b[3] and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    for waves in (1, 7):
        with L.probe() as pr:
            pr.set("dreg_render_set_waves", waves, 0)
            c = R.render_image(f, occ, rays, AABB, **kw)
        assert c[3] == a[3] and all(torch.equal(x, y) for x, y in zip(a[:3], c[:3])), waves


def test_render_image_drop_in_shapes(block):
    f, occ, _, _ = block
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    with torch.no_grad():
        rgb, opac, depth, ns = R.render_image(f, occ, rays, torch.tensor(AABB), render_step_size=0.02, test_chunk_size=100)
    assert rgb.shape == (H, W, 3) and opac.shape == (H, W, 1) and depth.shape == (H, W, 1) and isinstance(ns, int) and ns > 0
    flat = R.Rays(rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3))
    rgb2, opac2, depth2, ns2 = R.render_image(f, occ, flat, AABB, render_step_size=0.02)
    assert rgb2.shape == (H * W, 3) and opac2.shape == (H * W, 1) and depth2.shape == (H * W, 1) and ns2 == ns
    assert torch.equal(rgb2.view(H, W, 3), rgb) and torch.equal(depth2.view(H, W, 1), depth)
    with pytest.raises(NotImplementedError):
        R.render_image(f, occ, flat, AABB, render_step_size=0.02, cone_angle=0.004)
    f.train()
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            R.render_image(f, occ, flat, AABB, render_step_size=0.02)
    finally:
        f.eval()


def _eval_helpers():
    spec = importlib.util.spec_from_file_location("_evalpipe", os.path.join(ROOT, "tests", "test_hip_eval_pipeline.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_eval_render_views_writes_the_reference_files(tmp_path):
    E = _eval_helpers()
    root, jdir, names = E._split(tmp_path, 1)
    common = ["--root_dir", str(root), "--json_dir", str(jdir), "--dataset", "objaverse", "--expname", "chain", "--precision", "fp32"]
    E._run([sys.executable, "eval_ngp_nerf.py", "--root_dir", str(root), "--dataset", "objaverse", "--multi_blocks"])
    sdir = root / "eval" / "chain" / "objaverse" / names[0]
    E._run([sys.executable, "eval_nerf_regtr.py"] + common)
    assert not sdir.exists() or not any(p.name.endswith("_images") for p in sdir.iterdir())
    out = E._run([sys.executable, "eval_nerf_regtr.py"] + common + ["--render_views"])
    ncam = 6 + 6                                 # the generated blocks carry six cameras each
    for prefix in ("gt", "aligned", "unaligned"):
        for i in range(ncam):
            for sub, size in ((f"{prefix}_src_images/rgb_{i}.png", (800, 800)), (f"{prefix}_tgt_images/rgb_{i}.png", (800, 800)),
                              (f"{prefix}_images/src_tgt_rgb_depth_{i}.png", (3200, 800))):
                assert Image.open(sdir / sub).size == size, sub
        assert not (sdir / f"{prefix}_images" / f"src_tgt_rgb_depth_{ncam}.png").exists()
        assert (sdir / f"{prefix}_src_tgt_rgb_depth.mp4").exists() or f"{prefix}: no ffmpeg on PATH" in out
    # the block is visible: not every pixel of every view is background
    assert any((np.asarray(Image.open(sdir / "unaligned_src_images" / f"rgb_{i}.png")) != 255).any() for i in range(ncam))
