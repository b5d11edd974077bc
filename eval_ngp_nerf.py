#!/usr/bin/env python3
"""Voxel-grid extraction from trained NeRF blocks on MI355X — drop-in for the `sample_points` part of the reference's
eval_ngp_nerf.py (:336-451, `--multi_blocks`): for every <root>/<dataset>/nerf_models/<scene>/block_k/model.pth write
voxel_grid.pt / voxel_mask.pt / voxel_point_cloud.ply and their density_voxel_* twins next to it.  Blocks are independent: ranks take blocks round-robin (replicas only).

The reference's other two jobs, for a scene trained by train_ngp_nerf.py (<root>/<scene> images, <root>/out/<expname>/[block_k/]model.pth), run INSTEAD of
the extraction when asked for:

    python eval_ngp_nerf.py --dataset objaverse --root_dir <images> --scene <id> --expname <id> [--multi_blocks] --eval_images --point_cloud [--normals]

  --eval_images   evaluate() (:159-244): held-out views rendered over white, PSNR / SSIM by the fused kernel (dreg_nerf_amd/image_metrics.py) ->
                  <root>/eval/<scene>/[block_k/]val/{rgb_test,rgb_gt,inv_depth_test}_i.png and metrics.json (no lpips key: DESIGN.md §3d)
  --point_cloud   generate_point_cloud() (:246-334): depth-range points of the training cameras -> point_cloud.ply next to the checkpoint

and, which the reference does on the host with skimage (utils.py:284-344, convert_sdf_samples_to_ply), for the blocks the extraction would visit (or --ckpt_path):

  --mesh [--mesh_resolution 256] [--mesh_level L]   the block's density iso-surface by the fused marching-cubes kernels -> mesh.ply next to the checkpoint"""
import glob
import os

import torch

from dreg_nerf_amd import ngp
from dreg_nerf_amd.checkpoint import CheckPointManager
from dreg_nerf_amd.config import config_parser


@torch.no_grad()
def extract_block(ckpt_path: str, dev, density_thre: float = 0.7):
    # the reference's two-pass load (eval_ngp_nerf.py:63-115): meta data, then the modules constructed from it
    meta = {k: None for k in ("aabb", "unbounded", "grid_resolution", "contraction_type",
                              "render_step_size", "alpha_thre", "cone_angle", "camera_poses")}
    mgr = CheckPointManager(verbose=False)
    mgr.load_no_config(ckpt_path, meta_data=meta, map_location="cpu")
    field = ngp.NGPradianceField(meta["aabb"], unbounded=bool(meta["unbounded"]))
    occ = ngp.OccupancyGrid(meta["aabb"], meta["grid_resolution"], meta["contraction_type"])
    mgr.load_no_config(ckpt_path, models={"model": field, "occupancy_grid": occ}, map_location="cpu")
    field = field.to(dev).eval()
    sg = ngp.SampleGrid(meta["aabb"], meta["grid_resolution"], meta["contraction_type"]).to(dev)
    sg.set_binary_fields(occ.binary.to(dev))
    res = int(sg.resolution[0])
    state = meta
    world, rgb, alpha, idx, dmask, smask = sg.query_radiance_and_density_from_camera(field, None, state, dev, density_thre)
    out_dir = os.path.dirname(ckpt_path)
    # the density-field twins first (eval_ngp_nerf.py:350-381), then the surface AND density set the registration dataset reads (:383-412)
    dgrid, dmask_idx = ngp.build_voxel_grid(world, rgb, alpha, idx, dmask, res)
    ngp.save_voxel_grid(out_dir, dgrid, dmask_idx, prefix="density_voxel", points=world[dmask], colors=rgb[dmask])
    keep = dmask & smask
    grid, mask = ngp.build_voxel_grid(world, rgb, alpha, idx, keep, res)
    ngp.save_voxel_grid(out_dir, grid, mask, points=world[keep], colors=rgb[keep])
    from dreg_nerf_amd import visibility
    visibility.OVERRUN.check(wait=True)      # a surface-label launch that hit its pass bound is an error of THIS block, raised before the next one
    return int(mask.shape[0])


def _png_u8(path: str, img_u8):
    from PIL import Image
    Image.fromarray(img_u8).save(path)


def _render_view(field, grid, meta, rays, bkgd):
    from dreg_nerf_amd import render
    return render.render_image(field, grid, rays, meta["aabb_host"], near_plane=meta.get("near_plane"), far_plane=meta.get("far_plane"),
                               render_step_size=float(meta["render_step_size"]), render_bkgd=bkgd, alpha_thre=float(meta.get("alpha_thre") or 0.0))


@torch.no_grad()
def evaluate_block(ckpt_path: str, val, scene: str, out_dir: str, dev, views_per_call: int = 32):
    """The reference's evaluate() (eval_ngp_nerf.py:159-244) for one block: render every held-out view of `val` (a SubjectImages) over white, PSNR and
    SSIM of all views through one fused call per `views_per_call` views (dreg_nerf_amd/image_metrics.py), val/rgb_test_i.png, rgb_gt_i.png (the kernel's
    uint8 copies), inv_depth_test_i.png and metrics.json under out_dir.  LPIPS is not computed.  Returns the metrics dict."""
    import numpy as np
    from dreg_nerf_amd import image_metrics as IM, render
    field, grid, meta = render.load_render_block(ckpt_path, dev)
    vdir = os.path.join(out_dir, "val")
    os.makedirs(vdir, exist_ok=True)
    bkgd = torch.ones(3)
    psnrs, ssims = [], []
    for lo in range(0, len(val), views_per_call):
        ids = range(lo, min(lo + views_per_call, len(val)))
        preds, gts, depths = [], [], []
        for i in ids:
            rays, pixels = val.view(i)
            rgb, _acc, depth, _n = _render_view(field, grid, meta, rays, bkgd)
            preds.append(rgb)
            gts.append(pixels)
            depths.append(depth[..., 0])
        m = IM.image_metrics(torch.stack(preds), torch.stack(gts), return_u8=True)
        psnrs += m["psnr"].cpu().tolist()
        ssims += m["ssim"].cpu().tolist()
        pred_u8, gt_u8 = m["pred_u8"].cpu().numpy(), m["gt_u8"].cpu().numpy()
        for k, i in enumerate(ids):
            _png_u8(os.path.join(vdir, f"rgb_test_{i}.png"), pred_u8[k])
            _png_u8(os.path.join(vdir, f"rgb_gt_{i}.png"), gt_u8[k])
            inv = render.colorize_depth(1.0 / np.maximum(depths[k].cpu().numpy(), 1e-6))
            _png_u8(os.path.join(vdir, f"inv_depth_test_{i}.png"), (np.clip(inv, 0.0, 1.0) * 255).astype(np.uint8))
    return IM.write_metrics_json(os.path.join(out_dir, "metrics.json"), scene, psnrs, ssims)


@torch.no_grad()
def generate_point_cloud(ckpt_path: str, K, width: int, height: int, dev, min_depth: float = 2.0, max_depth: float = 6.0, normals: bool = False):
    """The reference's generate_point_cloud (eval_ngp_nerf.py:246-334): the block rendered over white from every training camera of the checkpoint
    (camera_poses) at the dataset's intrinsics; pixels with min_depth <= depth <= max_depth become points o + d * depth with the rendered colour,
    in camera-then-pixel order, written to point_cloud.ply next to the checkpoint.  Returns the number of points."""
    from dreg_nerf_amd import image_metrics as IM, render, vis_dump
    field, grid, meta = render.load_render_block(ckpt_path, dev)
    bkgd = torch.ones(3)

    def views():
        for c2w in torch.as_tensor(meta["camera_poses"]).float():
            rays = render.pixel_rays(c2w.to(dev), K, width, height)
            rgb, _acc, depth, _n = _render_view(field, grid, meta, rays, bkgd)
            yield rays.origins, rays.viewdirs, depth, rgb

    points, colors = IM.point_cloud_from_views(views(), min_depth, max_depth)
    path = os.path.join(os.path.dirname(ckpt_path), "point_cloud.ply")
    nrm = None
    if normals:          # --normals: the field's own surface normals at the points (the density gradient); the file is unchanged without the flag
        nrm = ngp.field_normals(field, points.float()).cpu().numpy()
    vis_dump.write_ply(path, points.float().cpu().numpy(), colors.float().cpu().numpy(), nrm)
    print(f"[INFO] Point Cloud Saved to {path}.", flush=True)
    return int(points.shape[0])


def _checkpoint_block_id(path: str):
    ngp.install_pickle_shims()
    try:
        snap = torch.load(path, map_location="cpu", weights_only=False, mmap=True)
    except (RuntimeError, ValueError):
        snap = torch.load(path, map_location="cpu", weights_only=False)
    return snap.get("block_id")


def block_checkpoints(cfg):
    """[(block id or None, checkpoint path)] and the number of blocks of the scene: --ckpt_path when given, else the trainer's layout
    <root>/out/<expname>/model.pth, or block_k/model.pth of every block_* directory with --multi_blocks."""
    if cfg.ckpt_path:
        if not cfg.multi_blocks:
            return [(None, cfg.ckpt_path)], 1
        base = os.path.dirname(os.path.dirname(os.path.abspath(cfg.ckpt_path)))
        k = _checkpoint_block_id(cfg.ckpt_path)
        if k is None:
            raise RuntimeError(f"{cfg.ckpt_path}: --multi_blocks needs a checkpoint with a block_id")
        return [(int(k), cfg.ckpt_path)], max(len(glob.glob(os.path.join(base, "block_*", ""))), int(k) + 1)
    base = os.path.join(cfg.root_dir, "out", cfg.expname)
    if not cfg.multi_blocks:
        return [(None, os.path.join(base, "model.pth"))], 1
    dirs = sorted(glob.glob(os.path.join(base, "block_*", "")), key=lambda d: int(os.path.basename(os.path.dirname(d)).split("_")[1]))
    if not dirs:
        raise FileNotFoundError(f"no block_* directory under {base}")
    return [(int(os.path.basename(os.path.dirname(d)).split("_")[1]), os.path.join(d, "model.pth")) for d in dirs], len(dirs)


def evaluate_scene(cfg, dev):
    """--eval_images / --point_cloud: the first two jobs of the reference's eval_ngp_nerf.py for one scene trained by train_ngp_nerf.py."""
    from dreg_nerf_amd.nerf_images import SubjectImages
    if not cfg.scene:
        raise SystemExit("--eval_images / --point_cloud need --scene")
    ckpts, n_blocks = block_checkpoints(cfg)
    for _, path in ckpts:
        if not os.path.exists(path):
            raise FileNotFoundError(f"Checkpoint path '{path}' does not exist!")
    val_sets = SubjectImages.load(cfg.dataset, cfg.root_dir, cfg.scene, "test", dev, cfg.multi_blocks, n_blocks)
    for k, path in ckpts:
        val = val_sets[k if k is not None else 0]
        out_dir = os.path.join(cfg.root_dir, "eval", cfg.scene, *([f"block_{k}"] if k is not None else []))
        os.makedirs(out_dir, exist_ok=True)
        if cfg.eval_images:
            res = evaluate_block(path, val, cfg.scene, out_dir, dev)
            print(f"{path}: {len(val)} views, psnr {res[cfg.scene]['psnr']:.3f} ssim {res[cfg.scene]['ssim']:.5f} -> {out_dir}/metrics.json", flush=True)
        if cfg.point_cloud:
            generate_point_cloud(path, val.K, val.WIDTH, val.HEIGHT, dev, normals=cfg.normals)


def mesh_checkpoints(cfg):
    """The checkpoints --mesh visits: --ckpt_path when given; else the registration layout the extraction reads; else the trainer's layout."""
    if cfg.ckpt_path:
        return [cfg.ckpt_path]
    found = sorted(glob.glob(os.path.join(cfg.root_dir, cfg.dataset, "nerf_models", cfg.scene or "*", "block_*", "model.pth")))
    return found or [p for _, p in block_checkpoints(cfg)[0] if os.path.exists(p)]


def main():
    cfg = config_parser()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", cfg.local_rank)))
    torch.cuda.set_device(dev)
    if cfg.mesh:                                 # surface meshes INSTEAD of the extraction; blocks round-robin over the ranks, as the extraction
        from dreg_nerf_amd import mesh
        for path in [p for i, p in enumerate(mesh_checkpoints(cfg)) if i % world == rank]:
            mesh.write_block_mesh(path, dev, cfg.mesh_resolution, cfg.mesh_level, log=lambda m: print(f"[rank {rank}] {m}", flush=True))
        return
    if cfg.eval_images or cfg.point_cloud:       # image metrics / depth point cloud of one trained scene; the grid extraction below is the default job
        evaluate_scene(cfg, dev)
        return
    pattern = os.path.join(cfg.root_dir, cfg.dataset, "nerf_models", cfg.scene or "*", "block_*", "model.pth")
    mine = [p for i, p in enumerate(sorted(glob.glob(pattern))) if i % world == rank]
    if os.environ.get("DREG_SERIAL_EXTRACT") == "1":       # the block-at-a-time form (what the reference does); same files, byte for byte
        for path in mine:
            print(f"[rank {rank}] {path}: {extract_block(path, dev)} voxels kept", flush=True)
        return
    # checkpoint reads, queries and file writes of different blocks overlapped (dreg_nerf_amd/eval_pipeline.py)
    from dreg_nerf_amd.eval_pipeline import ExtractionPipeline
    with ExtractionPipeline(dev) as pipe:
        done = []
        for ex in pipe.run(mine):
            done.append(ex)
            while len(done) > 4:            # report a few blocks behind the GPU: reading a count back waits for that block's query only
                e = done.pop(0)
                print(f"[rank {rank}] {e.path}: {e.kept()} voxels kept", flush=True)
        for e in done:
            print(f"[rank {rank}] {e.path}: {e.kept()} voxels kept", flush=True)


if __name__ == "__main__":
    main()
