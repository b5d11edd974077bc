#!/usr/bin/env python3
"""Evaluate NeRF registration on MI355X — drop-in for the metric part of the reference's eval_nerf_regtr.py
(:224-301; with --dump_outputs also its per-scene transformation_est.json and PLY point clouds, :313-438; with --render_views the renders of
both NeRF blocks under the ground-truth, predicted and no alignment, :113-172 / :345-369; with --render_merged, which the reference lacks,
both blocks rendered as one scene under the ground-truth and the predicted pose and merged_metrics.json; with --merged_mesh the two
blocks' surface meshes in one frame under both poses, merged_mesh_pred.ply / merged_mesh_gt.ply; with --merged_mesh_field the pair meshed as ONE density field, one closed surface per pose,
merged_field_mesh_pred.ply / merged_field_mesh_gt.ply / merged_field_mesh.json; with --register_scene every scene registered as a
whole — all ordered pairs of its blocks, pose synchronisation, scene_metrics_<split>.json — and with --render_scene all its blocks rendered as one
scene under the ground-truth and the synchronised poses; with --scene_mesh_field all its blocks meshed as ONE density field under both
pose sets, scene_field_mesh_gt.ply / scene_field_mesh_aligned.ply / scene_field_mesh.json; with --scene_voxel_grid all its blocks
extracted as ONE voxel grid in a block's own format under both pose sets, scene_voxel_grid_{gt,aligned}.pt / scene_voxel_mask_{gt,aligned}.pt /
scene_voxel_grid.json; with --merge_scene all its blocks distilled into ONE NeRF block under both pose sets,
merged_block_{gt,aligned}/model.pth / merged_block.json; with --refine_scene every scene's synchronised poses refined jointly by
point-to-plane ICP over all block pairs at once, scene_refined_metrics_<split>.json, the scene products then taking the refined poses, DESIGN.md §3n;
with --photo_refine every scene's pose refined photometrically through the field's input gradients, photo_refined_metrics_<split>.json): per-scene RRE/RTE + forward time (with a device sync, unlike the reference — quirk Q13) written to
<root>/eval/<expname>/<dataset>/metrics_<split>.json with the reference's schema.  Scenes are sharded over ranks
when launched with torch.distributed.run (replicas only, results gathered on rank 0)."""
import json
import os
import time

import torch
import torch.distributed as dist

from dreg_nerf_amd import eval_shard as ES
from dreg_nerf_amd import fgr, vis_dump
from dreg_nerf_amd import losses as LS
from dreg_nerf_amd.checkpoint import CheckPointManager
from dreg_nerf_amd.config import config_parser
from dreg_nerf_amd.dataset import NeRFRegDataset, SyntheticRegDataset
from dreg_nerf_amd.regtr import NeRFRegTr


def _points(data, side):
    """World coordinates of the occupied voxels of one block = the voxel point cloud the reference reads from its PLY."""
    if side + "_sparse" in data:
        return data[side + "_sparse"].vals[:, :3].float()
    g = data[side + "_xyz_rgba"]
    g = g.squeeze(0) if g.dim() == 6 else g
    m = data[side + "_mask"]
    m = m.squeeze(0) if m.dim() == 2 else m
    return g[:, :3].permute(0, 3, 4, 2, 1).reshape(-1, 3)[m].float()      # same flattening as nerf_regtr.py:144-147


def _row(err, dt):
    return {"R_mean": float(err["R_error_mean"]), "t_mean": float(err["t_error_mean"]), "R_med": float(err["R_error_med"]), "t_med": float(err["t_error_med"]), "time": dt}


def refine_scene_pose(cfg, data, pred, dev, refiner=None, log=print, with_pose=False):
    """--refine_pose for one scene: the row of refined_metrics_{split}.json (with_pose: and the pose [1,3,4] it scores).  Target normals from the
    target block's field when --icp_normals field and its checkpoint is on disk, else by PCA (a printed line says so)."""
    from dreg_nerf_amd import icp
    field = None
    tp = data.get("tgt_nerf_path", "")
    if cfg.icp_normals == "field" and tp and os.path.exists(tp):
        from dreg_nerf_amd.visibility import load_block
        field = load_block(tp, dev)[0]
        if field.unbounded:
            field = None
    row, pose = icp.refine_scene(_points(data, "src"), _points(data, "tgt"), pred["pose"][-1], data["pose"], field, cfg.icp_max_dist, cfg.icp_iters,
                                 refiner=refiner, log=lambda m: log(m, flush=True), scene=str(data["scene"]))
    return (row, pose) if with_pose else row


def photo_refine_scenes(cfg, jobs, dev, refine=None, log=print):
    """--photo_refine: the photometric refinement of every scene of `jobs` = [(scene, source checkpoint, target checkpoint, start pose [3,4], gt pose)],
    after the normal pass: {scene: row of photo_refined_metrics_{split}.json}.  A scene whose blocks are not on disk is skipped with a
    printed line.  refine(src_path, tgt_path, start, gt) -> (row, pose) replaces photo_refine.photo_refine_scene (tests)."""
    rows = {}
    for scene, sp, tp, start, gt in jobs:
        if not (sp and tp and os.path.exists(sp) and os.path.exists(tp)):
            log(f"{scene}: no NeRF blocks on disk, pose not refined photometrically", flush=True)
            continue
        if refine is None:
            from dreg_nerf_amd.photo_refine import photo_refine_scene
            row, _ = photo_refine_scene(sp, tp, start, gt, cfg.dataset, dev, cfg.photo_iters, cfg.photo_rays, cfg.photo_lr, cfg.photo_depth_weight, cfg.seed)
        else:
            row, _ = refine(sp, tp, start, gt)
        rows[scene] = row
        log(f"{scene}: photometric refinement, {row['iterations']} iterations: R {row['R_start']:.3f} -> {row['R_mean']:.3f} deg, "
            f"t {row['t_start']:.4f} -> {row['t_mean']:.4f}", flush=True)
    return rows


def write_photo_refined(d, split, photo_rows, log=print):
    """photo_refined_metrics_{split}.json: icp.write_refined_metrics' schema (ES.summary's layout), every row with its start errors and iterations."""
    from dreg_nerf_amd import icp
    out = icp.write_refined_metrics(os.path.join(d, f"photo_refined_metrics_{split}.json"), photo_rows)
    n = max(len(photo_rows), 1)
    log(f"photometric refinement, {len(photo_rows)} scenes: R_mean {sum(r['R_start'] for r in photo_rows.values()) / n:.3f} -> {out['R_mean']:.3f} deg, "
        f"t_mean {sum(r['t_start'] for r in photo_rows.values()) / n:.4f} -> {out['t_mean']:.4f} -> {d}/photo_refined_metrics_{split}.json", flush=True)
    return out


def write_refined(d, split, rows, refined_rows, log=print):
    """refined_metrics_{split}.json (ES.summary's schema, fitness and status per scene) and RRE / RTE before and after."""
    from dreg_nerf_amd import icp
    out = icp.write_refined_metrics(os.path.join(d, f"refined_metrics_{split}.json"), refined_rows)
    before = ES.summary({k: rows[k] for k in refined_rows if k in rows})
    kept = sum(1 for r in refined_rows.values() if r["status"] in (2, 3))
    log(f"ICP refinement, {len(refined_rows)} scenes ({kept} kept the predicted pose): R_mean {before['R_mean']:.3f} -> {out['R_mean']:.3f} deg, "
        f"t_mean {before['t_mean']:.4f} -> {out['t_mean']:.4f} -> {d}/refined_metrics_{split}.json", flush=True)
    return out


def ransac_scene_pose(cfg, data, pred, estimator=None):
    """--ransac_pose for one scene: (row of ransac_metrics_{split}.json, pose [1,3,4]) from the last layer's predicted correspondences (fused
    RANSAC kernels + consensus refits).  A scene without a valid hypothesis (status 2) keeps the predicted pose."""
    from dreg_nerf_amd import pose_ransac
    return pose_ransac.ransac_scene(pred, data["pose"], cfg.ransac_thresh, cfg.ransac_hyps, cfg.ransac_seed, cfg.ransac_min_overlap, estimator=estimator)


def write_ransac(d, split, rows, ransac_rows, ransac_refined_rows=None, log=print):
    """ransac_metrics_{split}.json (ES.summary's schema; inliers, inlier_ratio and status per scene), with --refine_pose also
    ransac_refined_metrics_{split}.json, and RRE / RTE of the Kabsch pose against the RANSAC pose."""
    from dreg_nerf_amd import icp, pose_ransac
    out = pose_ransac.write_ransac_metrics(os.path.join(d, f"ransac_metrics_{split}.json"), ransac_rows)
    before = ES.summary({k: rows[k] for k in ransac_rows if k in rows})
    kept = sum(1 for r in ransac_rows.values() if r["status"] == 2)
    log(f"RANSAC pose, {len(ransac_rows)} scenes ({kept} kept the predicted pose): Kabsch R_mean {before['R_mean']:.3f} deg, t_mean {before['t_mean']:.4f} | "
        f"RANSAC R_mean {out['R_mean']:.3f} deg, t_mean {out['t_mean']:.4f} -> {d}/ransac_metrics_{split}.json", flush=True)
    if ransac_refined_rows:
        ro = icp.write_refined_metrics(os.path.join(d, f"ransac_refined_metrics_{split}.json"), ransac_refined_rows)
        log(f"ICP from the RANSAC pose, {len(ransac_refined_rows)} scenes: R_mean {ro['R_mean']:.3f} deg, t_mean {ro['t_mean']:.4f} "
            f"-> {d}/ransac_refined_metrics_{split}.json", flush=True)
    return out


def register_scenes(cfg, ds, model, dev, rank=0, world=1, pair_fn=None, renderer=None, metrics=None, log=print, refiner=None, refined_rows=None):
    """--register_scene [--scene_robust] [--refine_scene] [--render_scene] [--scene_mesh_field] [--scene_voxel_grid]: this rank's scenes registered as WHOLE scenes (dreg_nerf_amd/scene_reg.py):
    {scene: row of scene_metrics_{split}.json}.  Runs after the normal pass; get_scene, the forward calls and the synchronisation draw from no
    random stream.  pair_fn / renderer / metrics are scene_reg's injection points (tests).  With --refine_scene every scene's synchronised poses
    are refined jointly (dreg_nerf_amd/scene_icp.py): its row of scene_refined_metrics_{split}.json goes into refined_rows, the scene
    products below take the refined poses, and the returned rows are those of the unflagged run.  refiner(scene, G_sync) -> (G [K,4,4], info)
    replaces scene_icp.refine_registered_scene (tests)."""
    from dreg_nerf_amd import scene_reg
    rows = {}
    refine = getattr(cfg, "refine_scene", False)
    for i in ES.my_scenes(len(ds), rank, world):
        scene = ds.get_scene(i)
        name = str(scene[0].get("scene", i))
        res = scene_reg.register_scene(model, scene, robust=cfg.scene_robust, pair_fn=pair_fn, eval_batch=max(cfg.eval_batch, 1), device=dev)
        rows[name] = scene_reg.scene_row(res, scene)
        if refine:   # the fine half at scene level: all pairs' point-to-plane residuals over the K - 1 free poses at once, from the synchronised poses
            from dreg_nerf_amd import scene_icp
            if refiner is not None:
                G_ref, info = refiner(scene, res["G"])
            else:
                G_ref, info = scene_icp.refine_registered_scene(scene, res["G"], dev, cfg.icp_max_dist, cfg.icp_iters, cfg.icp_normals, log=lambda m: log(m, flush=True))
            row = scene_icp.refined_scene_row(res, G_ref, info, scene)
            if refined_rows is not None:
                refined_rows[name] = row
            kept = info["status"] in (2, 3)
            log(f"{name}: joint ICP of {len(scene)} blocks, status {info['status']} after {info['iterations']} iterations, fitness {info['fitness']:.3f}: R_mean "
                f"{row['R_mean_sync']:.3f} -> {row['R_mean']:.3f} deg, t_mean {row['t_mean_sync']:.4f} -> {row['t_mean']:.4f}; the scene products take the "
                f"{'synchronised poses (the refinement ended with status 2 or 3)' if kept else 'refined poses'}", flush=True)
            if not kept:
                res = {**res, "G": torch.as_tensor(G_ref).double().cpu()}
        if cfg.render_scene:
            paths = [b.get("nerf_path", "") for b in scene]
            if renderer is not None or all(p and os.path.exists(p) for p in paths):
                scene_dir = os.path.join(cfg.root_dir, "eval", cfg.expname, cfg.dataset or "synthetic", name)
                mm = scene_reg.render_registered_scene(scene_dir, scene, scene_reg.ground_truth(scene), res["G"], cfg.dataset, dev, renderer=renderer, metrics=metrics)
                log(f"{name}: scene render of {len(scene)} blocks, aligned vs gt PSNR {mm['psnr_mean']:.2f} dB, SSIM {mm['ssim_mean']:.4f}", flush=True)
            else:
                log(f"{name}: no NeRF blocks on disk, scene not rendered", flush=True)
        if cfg.scene_mesh_field:   # all blocks as ONE density field (the scene --render_scene renders), one closed surface per pose set
            paths = [b.get("nerf_path", "") for b in scene]
            if all(p and os.path.exists(p) for p in paths):
                from dreg_nerf_amd.scene_field import registered_scene_mesh
                scene_dir = os.path.join(cfg.root_dir, "eval", cfg.expname, cfg.dataset or "synthetic", name)
                st = registered_scene_mesh(scene_dir, scene, scene_reg.ground_truth(scene), res["G"], cfg.dataset, dev, cfg.mesh_resolution, cfg.mesh_level)["stats"]
                log(f"{name}: scene field mesh of {st['K']} blocks, aligned V {st['aligned']['V']} F {st['aligned']['F']} area {st['aligned']['area']:.4f} volume "
                    f"{st['aligned']['volume']:.4f}, gt V {st['gt']['V']} F {st['gt']['F']} area {st['gt']['area']:.4f} volume {st['gt']['volume']:.4f} -> "
                    f"{scene_dir}/scene_field_mesh_{{aligned,gt}}.ply", flush=True)
            else:
                log(f"{name}: no NeRF blocks on disk, scene field mesh not written", flush=True)
        if getattr(cfg, "scene_voxel_grid", False):   # all blocks as ONE voxel grid in a block's own format: again an input of the network
            paths = [b.get("nerf_path", "") for b in scene]
            if all(p and os.path.exists(p) for p in paths):
                from dreg_nerf_amd.scene_grid import registered_scene_grid
                scene_dir = os.path.join(cfg.root_dir, "eval", cfg.expname, cfg.dataset or "synthetic", name)
                st = registered_scene_grid(scene_dir, scene, scene_reg.ground_truth(scene), res["G"], cfg.dataset, dev, cfg.scene_grid_resolution)["stats"]
                log(f"{name}: scene voxel grid of {st['K']} blocks at {st['resolution']}, kept cells aligned {st['aligned']['kept']} gt {st['gt']['kept']}, "
                    f"IoU {st['iou']:.4f} -> {scene_dir}/scene_voxel_grid_{{aligned,gt}}.pt", flush=True)
            else:
                log(f"{name}: no NeRF blocks on disk, scene voxel grid not written", flush=True)
        if getattr(cfg, "merge_scene", False):   # all blocks distilled into ONE NeRF block: a model.pth every single-block consumer accepts
            paths = [b.get("nerf_path", "") for b in scene]
            if all(p and os.path.exists(p) for p in paths):
                from dreg_nerf_amd.scene_merge import merge_registered_scene
                scene_dir = os.path.join(cfg.root_dir, "eval", cfg.expname, cfg.dataset or "synthetic", name)
                st = merge_registered_scene(scene_dir, scene, scene_reg.ground_truth(scene), res["G"], cfg.dataset, dev, cfg.merge_iterations, cfg.merge_points)["stats"]
                log(f"{name}: {st['K']} blocks merged into one in {st['steps']} steps of {st['points']} points, final loss aligned {st['aligned']['final_loss']:.5f} "
                    f"gt {st['gt']['final_loss']:.5f} -> {scene_dir}/merged_block_{{aligned,gt}}/model.pth", flush=True)
            else:
                log(f"{name}: no NeRF blocks on disk, scene not merged", flush=True)
    return rows


def write_scenes(d, split, scene_rows, log=print):
    """scene_metrics_{split}.json and the synchronised poses' RRE / RTE beside the direct edges'."""
    from dreg_nerf_amd import scene_reg
    out = scene_reg.write_scene_metrics(os.path.join(d, f"scene_metrics_{split}.json"), scene_rows)
    log(f"scene registration, {len(scene_rows)} scenes: synchronised R_mean {out['R_mean']:.3f} deg, t_mean {out['t_mean']:.4f} | direct edges R_mean "
        f"{out['R_mean_direct']:.3f} deg, t_mean {out['t_mean_direct']:.4f} -> {d}/scene_metrics_{split}.json", flush=True)
    return out


def write_scenes_refined(d, split, refined_rows, log=print):
    """scene_refined_metrics_{split}.json and RRE / RTE of the synchronised poses beside the jointly refined ones."""
    from dreg_nerf_amd import scene_icp
    out = scene_icp.write_scene_refined_metrics(os.path.join(d, f"scene_refined_metrics_{split}.json"), refined_rows)
    kept = sum(1 for r in refined_rows.values() if r["status"] in (2, 3))
    log(f"joint scene ICP, {len(refined_rows)} scenes ({kept} kept the synchronised poses): R_mean {out['R_mean_sync']:.3f} -> {out['R_mean']:.3f} deg, "
        f"t_mean {out['t_mean_sync']:.4f} -> {out['t_mean']:.4f} -> {d}/scene_refined_metrics_{split}.json", flush=True)
    return out


def init_distributed(local_rank: int):
    """One process per GPU under torch.distributed.run: RCCL ('nccl' on ROCm).  DREG_EVAL_BACKEND=gloo with DREG_EVAL_ONE_GPU=1 is the test hook bench.py
    has too — several ranks on the one GPU of a test box exercise the sharding and the gather (tests/test_hip_eval_pipeline.py); never a measurement."""
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("DREG_EVAL_BACKEND", "nccl")
    if os.environ.get("DREG_EVAL_ONE_GPU") == "1":
        local_rank = 0
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group(backend)
    return local_rank


def implied_flags(cfg):
    """The flags other flags imply: the scene render, the scene mesh and the scene voxel grid need the synchronised poses, so --render_scene,
    --scene_mesh_field, --scene_voxel_grid, --merge_scene and --refine_scene each imply --register_scene (and its scene_metrics file)."""
    if (cfg.render_scene or cfg.scene_mesh_field or getattr(cfg, "scene_voxel_grid", False) or getattr(cfg, "merge_scene", False) or
            getattr(cfg, "refine_scene", False)):
        cfg.register_scene = True
    return cfg


def main():
    cfg = implied_flags(config_parser())
    if cfg.register_scene and cfg.synthetic > 0 and not 2 <= cfg.synthetic_blocks <= 4:
        raise SystemExit(f"--synthetic_blocks {cfg.synthetic_blocks}: a synthetic scene has 2 to 4 blocks")      # before the normal pass, not after it
    import random
    import numpy as np
    random.seed(cfg.seed)            # setup_seed(config.seed) of the reference (eval_nerf_regtr.py:462, conerf/utils/utils.py:21-26): the block order of
    np.random.seed(cfg.seed)         # every scene (quirk Q15) and, with --extract_grids, the extraction's jitter (quirk Q11) are reproducible
    torch.manual_seed(cfg.seed)
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", cfg.local_rank))
    if world > 1:
        local_rank = init_distributed(local_rank)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    split = "test"
    ds = SyntheticRegDataset(cfg.synthetic, cfg.synthetic_res, split) if cfg.synthetic > 0 else \
        NeRFRegDataset(cfg.root_dir, cfg.json_dir, cfg.dataset, split, sparse=True, device=dev,
                       require_grids=not cfg.extract_grids)
    model = NeRFRegTr(cfg.position_embedding_type, cfg.position_embedding_dim, cfg.position_embedding_scaling,
                      cfg.num_downsample, precision=cfg.precision).to(dev).eval()
    ckpt_path = cfg.ckpt_path or os.path.join(cfg.root_dir, "out", cfg.expname, "model.pth")
    if CheckPointManager(verbose=rank == 0).load_no_config(ckpt_path, models={"model": model}, map_location=dev) == 0 and not os.path.exists(ckpt_path):
        print(f"[WARNING] no checkpoint at {ckpt_path}: evaluating random-init weights", flush=True)
    rows, fgr_rows, refined_rows = {}, {}, {}
    photo_jobs = []
    ransac_rows, ransac_refined_rows = {}, {}
    per_scene_extras = cfg.dump_outputs or cfg.fgr_baseline or cfg.render_views or cfg.render_merged or cfg.merged_mesh or cfg.merged_mesh_field
    mine = ES.my_scenes(len(ds), rank, world)
    # every rank consumes the block-order draws of ALL scenes in scene order: a scene's source / target assignment is then the one-rank run's,
    # whatever the rank count — the gathered metrics file does not depend on the sharding (dreg_nerf_amd/eval_shard.py)
    order_of = ES.block_orders(ds) if cfg.synthetic == 0 else {}
    if cfg.extract_grids and cfg.synthetic == 0:
        # BASELINE.json configs[4] in one process: this rank's scenes go through grid extraction (the reference's eval_ngp_nerf.py files are written) and are
        # registered from the device-resident grids, extraction of later scenes overlapping registration of earlier ones (dreg_nerf_amd/eval_pipeline.py)
        from dreg_nerf_amd.eval_pipeline import extract_and_register
        scenes = []
        for i in mine:
            sm = ds.meta[i]
            ids = order_of[i]                        # which block is the source: as the dataset draws it (quirk Q15)
            s, t = sm["blocks"][ids[0]], sm["blocks"][ids[1]]
            scenes.append((sm["scene"], os.path.join(s["dir"], "model.pth"), os.path.join(t["dir"], "model.pth"), t["transform"] @ torch.linalg.inv(s["transform"])))
        got, tm = extract_and_register(scenes, model, dev, batch_pairs=max(cfg.eval_batch, 1))
        rows = {k: {q: v[q] for q in ("R_mean", "t_mean", "R_med", "t_med", "time")} for k, v in got.items()}
        if rank == 0:
            print(f"extracted {tm['blocks']} blocks ({tm['bytes_written'] / 1e9:.2f} GB of grid files) and registered {len(rows)} pairs", flush=True)
        mine = []
        if cfg.render_views and rank == 0:
            print("--render_views: the scenes registered by --extract_grids are not rendered (run without --extract_grids for the renders)", flush=True)
    with torch.no_grad():
        step = 1 if per_scene_extras else max(cfg.eval_batch, 1)
        for b0 in range(0, len(mine), step):
            # `eval_batch` pairs per call (NeRFRegTr.forward_batch; the reference evaluates one pair per call — --eval_batch 1): samples are drawn in scene order on
            # this thread, so the block order a scene gets (quirk Q15) does not depend on the batch size
            batch = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in (ds.get(i, block_order=order_of[i]) if i in order_of else ds[i]).items()}
                     for i in mine[b0:b0 + step]]
            torch.cuda.synchronize()
            t0 = time.time()
            preds = model.forward_batch(batch)
            torch.cuda.synchronize()
            dt = (time.time() - t0) / len(batch)     # forward time per pair (with a device sync, unlike the reference — quirk Q13)
            model.check_inputs()      # a grid with values outside its voxel_mask (the row-list stem would have dropped them) is an error of THESE scenes
            for data, pred in zip(batch, preds):
                rows[data["scene"]] = _row(LS.evaluate_camera_alignment(pred["pose"][-1], data["pose"]), dt)
                start = pred["pose"][-1]
                if cfg.refine_pose:    # the "fine" half: point-to-plane ICP from the predicted pose (refine_registration, global_registration.py:85-93);
                    refined_rows[data["scene"]], start = refine_scene_pose(cfg, data, pred, dev, with_pose=True)      # the forward calls and their batches are the unflagged run's
                if cfg.photo_refine:   # run after the pass (below), from the ICP-refined pose when there is one, else from the predicted pose
                    photo_jobs.append((data["scene"], data.get("src_nerf_path", ""), data.get("tgt_nerf_path", ""),
                                       start.detach().reshape(3, 4).double().cpu(), data["pose"].detach().reshape(-1, 4)[:3].double().cpu()))
                if cfg.ransac_pose:    # the robust estimate from the same prediction's correspondences; nothing above reads it
                    ransac_rows[data["scene"]], rp = ransac_scene_pose(cfg, data, pred)
                    if cfg.refine_pose:
                        ransac_refined_rows[data["scene"]] = refine_scene_pose(cfg, data, {"pose": rp[None]}, dev)
            if not per_scene_extras:
                continue
            data, pred = batch[0], preds[0]
            scene_dir = os.path.join(cfg.root_dir, "eval", cfg.expname, cfg.dataset or "synthetic", str(data["scene"]))
            if cfg.dump_outputs:   # the reference's per-scene files (eval_nerf_regtr.py:313-321, 369-438; the renders are --render_views)
                cams = [None, None]
                sp, tp = data.get("src_nerf_path", ""), data.get("tgt_nerf_path", "")
                if sp and tp and os.path.exists(sp) and os.path.exists(tp):       # camera_poses of the two NeRF blocks (train_ngp_nerf.py:187-209)
                    from dreg_nerf_amd.visibility import load_block
                    cams = [load_block(q, dev)[2]["camera_poses"] for q in (sp, tp)]
                vis_dump.dump_scene_outputs(scene_dir, pred, data["pose"], cams[0], cams[1])
            if cfg.render_views:   # render_videos of the reference (eval_nerf_regtr.py:113-172, 345-369): gt / aligned / unaligned renders of both blocks
                sp, tp = data.get("src_nerf_path", ""), data.get("tgt_nerf_path", "")
                if sp and tp and os.path.exists(sp) and os.path.exists(tp):
                    from dreg_nerf_amd.render import render_scene_views
                    render_scene_views(scene_dir, sp, tp, data["pose"][0], pred["pose"][-1][0], cfg.dataset, dev)
                else:
                    print(f"{data['scene']}: no NeRF blocks on disk, views not rendered", flush=True)
            if cfg.render_merged:  # both blocks as ONE scene under the gt and the predicted pose, and what the pose error costs on screen
                sp, tp = data.get("src_nerf_path", ""), data.get("tgt_nerf_path", "")
                if sp and tp and os.path.exists(sp) and os.path.exists(tp):
                    from dreg_nerf_amd.render import render_scene_merged
                    mm = render_scene_merged(scene_dir, sp, tp, data["pose"][0], pred["pose"][-1][0], cfg.dataset, dev)
                    print(f"{data['scene']}: merged render, aligned vs gt PSNR {mm['psnr_mean']:.2f} dB, SSIM {mm['ssim_mean']:.4f}", flush=True)
                else:
                    print(f"{data['scene']}: no NeRF blocks on disk, merged scene not rendered", flush=True)
            if cfg.merged_mesh:    # both blocks' surfaces in the target frame under the predicted and the known pose (same pose conventions and skip rule as --render_merged)
                sp, tp = data.get("src_nerf_path", ""), data.get("tgt_nerf_path", "")
                if sp and tp and os.path.exists(sp) and os.path.exists(tp):
                    from dreg_nerf_amd.mesh import merged_scene_mesh
                    mm = merged_scene_mesh(scene_dir, sp, tp, data["pose"][0], pred["pose"][-1][0], dev, cfg.mesh_resolution, cfg.mesh_level)
                    print(f"{data['scene']}: merged mesh, source V {mm['src']['verts'].shape[0]} F {mm['src']['faces'].shape[0]}, target V {mm['tgt']['verts'].shape[0]} "
                          f"F {mm['tgt']['faces'].shape[0]} -> {scene_dir}/merged_mesh_{{pred,gt}}.ply", flush=True)
                else:
                    print(f"{data['scene']}: no NeRF blocks on disk, merged mesh not written", flush=True)
            if cfg.merged_mesh_field:   # the pair as ONE density field (the scene --render_merged renders), one closed surface per pose
                sp, tp = data.get("src_nerf_path", ""), data.get("tgt_nerf_path", "")
                if sp and tp and os.path.exists(sp) and os.path.exists(tp):
                    from dreg_nerf_amd.pair_field import merged_field_scene_mesh
                    st = merged_field_scene_mesh(scene_dir, sp, tp, data["pose"][0], pred["pose"][-1][0], dev, cfg.mesh_resolution, cfg.mesh_level)["stats"]
                    print(f"{data['scene']}: merged field mesh, pred V {st['pred']['V']} F {st['pred']['F']} area {st['pred']['area']:.4f} volume {st['pred']['volume']:.4f}, "
                          f"gt V {st['gt']['V']} F {st['gt']['F']} area {st['gt']['area']:.4f} volume {st['gt']['volume']:.4f} -> {scene_dir}/merged_field_mesh_{{pred,gt}}.ply",
                          flush=True)
                else:
                    print(f"{data['scene']}: no NeRF blocks on disk, merged field mesh not written", flush=True)
            if cfg.fgr_baseline:   # the reference's baseline on the two voxel point clouds (global_registration.py:96-116)
                T, sec = fgr.run_registration(_points(data, "src"), _points(data, "tgt"))
                e = LS.evaluate_camera_alignment(T[None].float(), data["pose"])
                fgr_rows[data["scene"]] = {"R_mean": float(e["R_error_mean"]), "t_mean": float(e["t_error_mean"]),
                                           "R_med": float(e["R_error_med"]), "t_med": float(e["t_error_med"]), "time": sec}
    photo_rows = {}
    if cfg.photo_refine:     # per scene, after the normal pass and apart from it (it needs autograd; the pass above runs under no_grad)
        photo_rows = ES.gather_rows(photo_refine_scenes(cfg, photo_jobs, dev), world)
    scene_rows, scene_refined_rows = {}, {}
    if cfg.register_scene:   # whole scenes, after the normal pass and apart from it: nothing above reads what this computes
        sds = SyntheticRegDataset(cfg.synthetic, cfg.synthetic_res, split, n_blocks=cfg.synthetic_blocks) if cfg.synthetic > 0 else ds
        with torch.no_grad():
            scene_rows = register_scenes(cfg, sds, model, dev, rank, world, refined_rows=scene_refined_rows)
    rows, fgr_rows, refined_rows = ES.gather_rows(rows, world), ES.gather_rows(fgr_rows, world), ES.gather_rows(refined_rows, world)
    if cfg.register_scene:
        scene_rows = ES.gather_rows(scene_rows, world)
        if getattr(cfg, "refine_scene", False):
            scene_refined_rows = ES.gather_rows(scene_refined_rows, world)
    if cfg.ransac_pose:
        ransac_rows, ransac_refined_rows = ES.gather_rows(ransac_rows, world), ES.gather_rows(ransac_refined_rows, world)
    if rank == 0:
        out = ES.summary(rows)
        d = os.path.join(cfg.root_dir, "eval", cfg.expname, cfg.dataset or "synthetic")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"metrics_{split}.json"), "w") as f:
            json.dump(out, f, indent=2)
        print(f"{len(rows)} scenes: R_mean={out['R_mean']:.3f} deg, t_mean={out['t_mean']:.4f} -> {d}/metrics_{split}.json", flush=True)
        if fgr_rows:
            fo = ES.summary(fgr_rows)
            with open(os.path.join(d, f"fgr_metrics_{split}.json"), "w") as f:
                json.dump(fo, f, indent=4)
            print(f"FGR baseline: R_mean={fo['R_mean']:.3f} deg, t_mean={fo['t_mean']:.4f} -> {d}/fgr_metrics_{split}.json", flush=True)
        if refined_rows:
            write_refined(d, split, rows, refined_rows)
        if ransac_rows:
            write_ransac(d, split, rows, ransac_rows, ransac_refined_rows)
        if photo_rows:
            write_photo_refined(d, split, photo_rows)
        if scene_rows:
            write_scenes(d, split, scene_rows)
        if scene_refined_rows:
            write_scenes_refined(d, split, scene_refined_rows)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
