"""GPU: the fused image-metrics kernel (csrc/image_metrics.hip, dreg_nerf_amd/image_metrics.py) against the fp64 restatement of its rule
(tests/image_metrics_restatement.py) on the case list defined there plus one 800x800x3 pair of views, its exact properties (identical images, uint8
copies, bit-identity between runs, guard values, null outputs), the reference's compute_psnr / compute_ssim drop-ins, and
eval_ngp_nerf.py --eval_images --point_cloud end to end on a generated block.

Bounds (image_metrics_restatement.bounds, derivations there): per case max(4 E_ref, floor), E_ref = the error of the fp32 torch restatement against
fp64 computed here on the CPU; capped at 4e-3 per map pixel, 1e-5 on the per-image SSIM, 1e-3 dB on PSNR."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import image_metrics_restatement as IR
from dreg_nerf_amd import image_metrics as IM
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import ngp
from dreg_nerf_amd import render as R
from dreg_nerf_amd import vis_dump
from dreg_nerf_amd.nerf_images import SubjectImages

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
ALL_CASES = IR.CASES + [IR.BIG_CASE]


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_kernel_matches_fp64_restatement(case):
    pred, gt, r64, _, bd = IR.reference(case)
    out = IM.image_metrics(pred.to(DEV), gt.to(DEV), return_map=True)
    got = {k: v.cpu() for k, v in out.items()}
    assert got["ssim"].shape == (case[2],) and got["ssim_map"].shape == pred.shape and got["ssim"].dtype == torch.float32
    e_map, e_ssim, e_psnr = IR.errors(got, r64)
    e_mse = ((got["mse"].double() - r64["mse"]).abs() / r64["mse"].clamp_min(1e-30)).max().item() if float(r64["mse"].max()) > 0 else float(got["mse"].abs().max())
    print(f"{case[0]}: map {e_map:.3e} (bound {bd['ssim_map']:.3e}) ssim {e_ssim:.3e} (bound {bd['ssim']:.3e}) psnr {e_psnr:.3e} dB (bound {bd['psnr']:.3e})"
          f" mse rel {e_mse:.3e}; E_ref {bd['e_ref']}")
    assert e_map <= bd["ssim_map"]
    assert e_ssim <= bd["ssim"]
    assert e_psnr <= bd["psnr"]
    assert e_mse <= 2.0 ** -22                                    # fp32 result of an fp64 mean: half an ulp, with room for the restatement's own sum


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (1, 33, 47, 3), (3, 64, 65, 1), (2, 800, 800, 3)], ids=lambda s: "x".join(map(str, s)))
def test_identical_images_are_exact(shape):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    out = IM.image_metrics(x, x.clone(), return_map=True)
    assert torch.equal(out["ssim"], torch.ones_like(out["ssim"])) and torch.equal(out["ssim_map"], torch.ones_like(x))
    assert torch.equal(out["mse"], torch.zeros_like(out["mse"]))
    assert torch.equal(out["psnr"], torch.full_like(out["psnr"], 60.0))


def test_uint8_copies_bitwise_runs_identical_and_layout():
    g = torch.Generator().manual_seed(11)
    pred = (torch.rand(3, 33, 47, 3, generator=g) * 1.4 - 0.2)       # values below 0 and above 1: the clamp
    pred[0, 0, 0, 0], pred[0, 0, 0, 1], pred[0, 0, 0, 2] = 1.0, 0.0, 254.999 / 255
    gt = torch.rand(3, 33, 47, 3, generator=g)
    p, t = pred.to(DEV), gt.to(DEV)
    a = IM.image_metrics(p, t, return_map=True, return_u8=True)
    assert a["pred_u8"].dtype == torch.uint8 and torch.equal(a["pred_u8"], (p.clamp(0, 1) * 255).to(torch.uint8))
    assert torch.equal(a["gt_u8"], (t.clamp(0, 1) * 255).to(torch.uint8))
    b = IM.image_metrics(p, t, return_map=True, return_u8=True)
    assert set(a) == set(b) == {"ssim", "mse", "psnr", "ssim_map", "pred_u8", "gt_u8"} and all(torch.equal(a[k], b[k]) for k in a)
    # a permuted (non-contiguous) input equals its contiguous copy; [H,W,C] is a batch of one; the map and the copies are optional
    pc, tc = p.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), t.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not pc.is_contiguous()
    c = IM.image_metrics(pc, tc, return_map=True, return_u8=True)
    assert all(torch.equal(a[k], c[k]) for k in a)
    one = IM.image_metrics(p[1], t[1])
    assert set(one) == {"ssim", "mse", "psnr"} and all(torch.equal(one[k], a[k][1:2]) for k in one)
    with pytest.raises(RuntimeError, match="no backward"):
        IM.image_metrics(p.clone().requires_grad_(), t)


def _raw_call(pred, gt, with_optional, guard=64):
    """The C ABI with guard bands behind every output and the workspace; returns the outputs and whether all bands survived."""
    lib = L.load()
    n, h, w, c = pred.shape
    nbytes = lib.dreg_image_metrics_workspace_bytes(n, h, w, c)
    assert nbytes == n * c * ((h + 31) // 32) * ((w + 31) // 32) * 16
    res = [torch.full((n + guard,), -7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    smap = torch.full((pred.numel() + guard,), -7.0, dtype=torch.float32, device=DEV)
    u8 = [torch.full((pred.numel() + guard,), 77, dtype=torch.uint8, device=DEV) for _ in range(2)]
    ws = torch.full((nbytes // 8 + guard,), -7.0, dtype=torch.float64, device=DEV)
    taps = (ctypes.c_float * 11)(*IM.gaussian_taps().tolist())
    opt = [smap.data_ptr(), u8[0].data_ptr(), u8[1].data_ptr()] if with_optional else [None, None, None]
    rc = lib.dreg_image_metrics(pred.data_ptr(), gt.data_ptr(), n, h, w, c, taps, res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), *opt,
                                ws.data_ptr(), nbytes, L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    bands = [bool((r[n:] == -7.0).all()) for r in res] + [bool((smap[pred.numel():] == -7.0).all()), bool((ws[nbytes // 8:] == -7.0).all())]
    bands += [bool((u[pred.numel():] == 77).all()) for u in u8]
    untouched = bool((smap == -7.0).all()) and all(bool((u == 77).all()) for u in u8)
    return [r[:n].clone() for r in res], smap[:pred.numel()].view(pred.shape), [u[:pred.numel()].view(pred.shape) for u in u8], all(bands), untouched


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 33, 47, 3), (1, 64, 65, 4), (2, 31, 96, 1)], ids=lambda s: "x".join(map(str, s)))
def test_guard_values_survive_and_null_outputs_are_accepted(shape):
    g = torch.Generator().manual_seed(2)
    pred, gt = torch.rand(shape, generator=g).to(DEV), torch.rand(shape, generator=g).to(DEV)
    want = IM.image_metrics(pred, gt, return_map=True, return_u8=True)
    res, smap, u8, bands_ok, _ = _raw_call(pred, gt, True)
    assert bands_ok
    assert torch.equal(res[0], want["ssim"]) and torch.equal(res[1], want["mse"]) and torch.equal(res[2], want["psnr"])
    assert torch.equal(smap, want["ssim_map"]) and torch.equal(u8[0], want["pred_u8"]) and torch.equal(u8[1], want["gt_u8"])
    res0, _, _, bands_ok, untouched = _raw_call(pred, gt, False)
    assert bands_ok and untouched and all(torch.equal(a, b) for a, b in zip(res, res0))
    lib = L.load()
    assert lib.dreg_image_metrics_workspace_bytes(1, 8, 8, 5) == 0 and lib.dreg_image_metrics_workspace_bytes(1, 0, 8, 3) == 0
    assert lib.dreg_image_metrics(pred.data_ptr(), gt.data_ptr(), 1, 8, 8, 5, None, None, None, None, None, None, None, None, 0, L.stream()) == -1


def test_reference_drop_ins():
    """compute_psnr(gt, pred, eps) / compute_ssim(gt, pred) of the reference's eval_ngp_nerf.py: [1,C,H,W] in, a 0-dim tensor / a float out."""
    case = IR.CASES[IR.CASE_NAMES.index("patch_33x47")]
    pred, gt, r64, _, bd = IR.reference(case)
    rgb, pixels = pred.to(DEV).permute(0, 3, 1, 2), gt.to(DEV).permute(0, 3, 1, 2)
    psnr = IM.compute_psnr(rgb, pixels)
    assert torch.is_tensor(psnr) and psnr.dim() == 0 and abs(psnr.item() - float(r64["psnr"][0])) <= bd["psnr"]
    s = IM.compute_ssim(pixels, rgb)
    assert isinstance(s, float) and abs(s - float(r64["ssim"][0])) <= bd["ssim"]
    no_eps = IM.compute_psnr(rgb, pixels, eps=0.0).item()
    assert no_eps == pytest.approx(-10 * math.log10(float(r64["mse"][0])), abs=1e-4) and no_eps > psnr.item()
    with pytest.raises(ValueError):
        IM.compute_ssim(pixels[0], rgb[0])


# ---------------------------------------------------------------------------------------------------------------- end to end
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
W, H = 64, 48
ANGLE_X = 2 * math.atan(0.5 * W / 60.0)                           # focal 60 px, as tests/test_hip_render.py's K
STEP = 0.02


def _block_state(seed=3, res=32, shell=(0.55, 1.05)):
    """The generated block of tests/test_hip_render.py::_block (random hash grid and MLPs, a thick occupancy shell) as modules on the host."""
    g = torch.Generator().manual_seed(seed)
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params[:3072] = torch.randn(3072, generator=g) * 1.0
        f.mlp_base.params[3072:] = torch.randn(f.mlp_base.params.numel() - 3072, generator=g)
        f.color_mlp.params.copy_(torch.randn(7168, generator=g) * 0.2)
    c = (torch.arange(res, dtype=torch.float32) + 0.5) / res * 3 - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    rad = torch.stack([X, Y, Z], -1).norm(dim=-1)
    occ = ngp.OccupancyGrid(AABB, res)
    occ._binary.copy_((rad > shell[0]) & (rad < shell[1]))
    return f, occ


def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target, up = torch.tensor(eye), torch.tensor(target), torch.tensor(up)
    back = torch.nn.functional.normalize(eye - target, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(up, back), dim=0)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, torch.linalg.cross(back, right), back, eye
    return c2w


def _render(field, grid, meta, rays):
    return R.render_image(field, grid, rays, meta["aabb_host"], near_plane=meta.get("near_plane"), far_plane=meta.get("far_plane"),
                          render_step_size=float(meta["render_step_size"]), render_bkgd=torch.ones(3), alpha_thre=float(meta.get("alpha_thre") or 0.0))


def test_eval_images_and_point_cloud_end_to_end(tmp_path):
    root, scene = tmp_path / "images", "scene_a"
    (root / scene).mkdir(parents=True)
    ckpt = root / "out" / scene / "model.pth"
    ckpt.parent.mkdir(parents=True)
    f, occ = _block_state()
    train_cams = torch.stack([_look_at((2.6, -1.9, 1.2), (0.0, 0.0, 0.0)), _look_at((-2.2, 2.4, -0.8), (0.0, 0.0, 0.0))])
    torch.save({"step": 1, "model": f.state_dict(), "occupancy_grid": occ.state_dict(), "aabb": AABB, "unbounded": False, "near_plane": None,
                "far_plane": None, "grid_resolution": 32, "contraction_type": ngp.ContractionType.AABB, "render_step_size": STEP, "alpha_thre": 0.0,
                "cone_angle": 0.0, "camera_poses": train_cams}, ckpt)
    field, grid, meta = R.load_render_block(str(ckpt), DEV)
    # three held-out views, written as an objaverse-layout scene: every 20th frame is the test split, so they sit at frames 0, 20 and 40 (the frames
    # between them, training views, reuse the same files)
    test_cams = [_look_at((2.4, 2.1, 0.9), (0.0, 0.0, 0.0)), _look_at((0.3, -3.2, 0.5), (0.0, 0.1, 0.0)), _look_at((2.8, 2.6, 0.4), (1.2, 1.2, 0.0))]
    # (rays through SubjectImages' own rule and the focal length the loader will derive from camera_angle_x: the evaluator then renders these very rays)
    focal = 0.5 * W / math.tan(0.5 * ANGLE_X)
    probe = SubjectImages(np.zeros((3, H, W, 4), np.uint8), torch.stack(test_cams).numpy(), focal, DEV)
    for k in range(3):
        rgb = _render(field, grid, meta, probe.view(k)[0])[0].cpu().numpy()
        rgba = np.concatenate([np.round(np.clip(rgb, 0, 1) * 255).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], axis=-1)
        Image.fromarray(rgba).save(root / scene / f"r_{k}.png")
    frames = [{"file_path": f"r_{(i // 20) if i % 20 == 0 else i % 3}", "transform_matrix": test_cams[(i // 20) if i % 20 == 0 else i % 3].tolist()}
              for i in range(41)]
    json.dump({"camera_angle_x": ANGLE_X, "frames": frames}, open(root / scene / "transforms.json", "w"))

    cmd = ["timeout", "-k", "10", "300", sys.executable, "eval_ngp_nerf.py", "--dataset", "objaverse", "--root_dir", str(root), "--scene", scene,
           "--expname", scene, "--eval_images", "--point_cloud"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    out_dir = root / "eval" / scene
    val = SubjectImages.load("objaverse", str(root), scene, "test", DEV)[0]
    assert len(val) == 3 and (val.WIDTH, val.HEIGHT) == (W, H)
    preds, gts = [], []
    for i in range(3):
        rays, pixels = val.view(i)
        preds.append(_render(field, grid, meta, rays)[0])
        gts.append(pixels)
    want = IM.image_metrics(torch.stack(preds), torch.stack(gts), return_u8=True)
    # files
    for i in range(3):
        for name in ("rgb_test", "rgb_gt", "inv_depth_test"):
            assert Image.open(out_dir / "val" / f"{name}_{i}.png").size == (W, H), (name, i)
        assert np.array_equal(np.asarray(Image.open(out_dir / "val" / f"rgb_test_{i}.png")), want["pred_u8"][i].cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(out_dir / "val" / f"rgb_gt_{i}.png")), np.asarray(Image.open(root / scene / f"r_{i}.png"))[..., :3])
    assert not (out_dir / "val" / "rgb_test_3.png").exists()
    # metrics.json: the reference's schema without lpips; every view's numbers are image_metrics of the re-render (the renderer is bit-identical)
    m = json.load(open(out_dir / "metrics.json"))
    assert set(m) == {scene} and set(m[scene]) == {"0", "1", "2", "psnr", "ssim"}
    psnr, ssim = want["psnr"].cpu().tolist(), want["ssim"].cpu().tolist()
    for i in range(3):
        assert m[scene][str(i)] == {"psnr": psnr[i], "ssim": ssim[i]}
    assert m[scene]["psnr"] == sum(psnr) / 3 and m[scene]["ssim"] == sum(ssim) / 3
    # the ground truth is the same render rounded to uint8: each value moves by at most 0.5 / 255, so mse <= (0.5 / 255)^2 and
    # psnr >= -10 log10((0.5 / 255)^2 + 1e-6) = 53.15 dB (less 1e-3 dB, the kernel's own bound); an unrelated image would sit near 10-20 dB
    level = -10 * math.log10((0.5 / 255) ** 2 + 1e-6)
    assert 53.1 < level < 53.2 and min(psnr) >= level - 1e-3 and max(psnr) < 60.0 and max(ssim) <= 1.0
    # point_cloud.ply next to the checkpoint: the training cameras' depth-range pixels, camera then pixel order
    xyz, rgb8 = vis_dump.read_ply(str(ckpt.parent / "point_cloud.ply"))
    views = []
    for c2w in train_cams:
        rays = R.pixel_rays(c2w.to(DEV), val.K, W, H)
        rgb, _, depth, _ = _render(field, grid, meta, rays)
        views.append((rays.origins, rays.viewdirs, depth, rgb))
    pts, cols = IM.point_cloud_from_views(views)
    depth_all = torch.cat([v[2].reshape(-1) for v in views])
    n_want = int(((depth_all >= 2.0) & (depth_all <= 6.0)).sum())
    assert 0 < n_want < depth_all.numel() and xyz.shape == (n_want, 3) and pts.shape[0] == n_want
    assert np.array_equal(xyz, pts.cpu().numpy().astype(np.float64))
    assert np.array_equal(rgb8, np.clip(np.round(cols.cpu().numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8))
    o = torch.cat([v[0].reshape(-1, 3) for v in views]).cpu().double()
    d = torch.cat([v[1].reshape(-1, 3) for v in views]).cpu().double()
    keep = ((depth_all >= 2.0) & (depth_all <= 6.0)).cpu()
    assert np.allclose(xyz, (o[keep] + d[keep] * depth_all.cpu().double()[keep, None]).numpy(), atol=1e-5)
