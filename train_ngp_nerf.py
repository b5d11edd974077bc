"""Train the Instant-NGP NeRF blocks of a scene (the reference's train_ngp_nerf.py, stage one of DReg-NeRF) on the library's kernels.

    python train_ngp_nerf.py --dataset objaverse --root_dir <images> --scene <id> --multi_blocks --min_num_blocks 2 --max_num_blocks 2 \
        --max_iterations 20000

Writes <root_dir>/out/<expname>/[block_k/]model.pth with the reference's checkpoint keys (train_ngp_nerf.py:187-209), which
visibility.load_block, eval_ngp_nerf.py and eval_nerf_regtr.py --render_views read.  With --data_split_json and no --scene every scene of the
split is trained, expname = scene.  AABB scenes of objaverse / nerf_synthetic only; the per-step rule is DESIGN.md §3c (dreg_nerf_amd/ngp_train.py)."""
import copy
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dreg_nerf_amd import ngp, ngp_train, render  # noqa: E402
from dreg_nerf_amd.checkpoint import CheckPointManager  # noqa: E402
from dreg_nerf_amd.config import config_parser  # noqa: E402
from dreg_nerf_amd.nerf_images import SubjectImages  # noqa: E402


def _png(path, img):
    from PIL import Image
    Image.fromarray((np.clip(img, 0.0, 1.0) * 255).astype(np.uint8)).save(path)


@torch.no_grad()
def validate(trainer: ngp_train.NGPTrainer, val: SubjectImages, out_dir: str) -> float:
    """Render every test view through render_image in eval mode (white background): mean PSNR; writes val/rgb_test_i.png, rgb_gt_i.png,
    depth_test_i.png and inv_depth_test_i.png."""
    field, grid = trainer.field, trainer.grid
    field.eval()
    grid.eval()
    vdir = os.path.join(out_dir, "val")
    os.makedirs(vdir, exist_ok=True)
    psnrs = []
    for i in range(len(val)):
        rays, pixels = val.view(i)
        rgb, _acc, depth, _n = render.render_image(field, grid, rays, trainer.aabb, render_step_size=trainer.render_step_size,
                                                   render_bkgd=trainer.bkgd, alpha_thre=trainer.alpha_thre)
        mse = torch.mean((rgb - pixels) ** 2)
        psnrs.append(float(-10.0 * torch.log10(mse)))
        d = depth[..., 0].cpu().numpy()
        _png(os.path.join(vdir, f"rgb_test_{i}.png"), rgb.cpu().numpy())
        _png(os.path.join(vdir, f"rgb_gt_{i}.png"), pixels.cpu().numpy())
        _png(os.path.join(vdir, f"depth_test_{i}.png"), render.colorize_depth(d))
        _png(os.path.join(vdir, f"inv_depth_test_{i}.png"), render.colorize_depth(1.0 / np.maximum(d, 1e-6)))
    field.train()
    grid.train()
    return float(np.mean(psnrs)) if psnrs else 0.0


def train_block(config, train_set: SubjectImages, val_set: SubjectImages, out_dir: str, device):
    aabb = [float(v) for v in config.aabb]
    field = ngp.NGPradianceField(aabb=aabb).to(device)
    grid = ngp.OccupancyGrid(roi_aabb=aabb, resolution=128, contraction_type=ngp.ContractionType.AABB).to(device)
    trainer = ngp_train.NGPTrainer(field, grid, train_set, aabb, config.max_iterations, backward=config.backward,
                                   opacity_loss_weight=config.opacity_loss_weight)
    os.makedirs(out_dir, exist_ok=True)
    ckpt = CheckPointManager(save_path=out_dir, max_to_keep=100, keep_checkpoint_every_n_hours=0.5)
    meta = {"aabb": aabb, "unbounded": False, "grid_resolution": 128, "contraction_type": ngp.ContractionType.AABB, "near_plane": None,
            "far_plane": None, "render_step_size": trainer.render_step_size, "alpha_thre": trainer.alpha_thre, "cone_angle": 0.0,
            "camera_poses": train_set.camtoworlds.cpu()}
    if train_set.current_block is not None:
        meta["block_id"] = train_set.current_block
    models = {"model": field, "occupancy_grid": grid}
    optims, scheds = {"optimizer": trainer.optimizer}, {"scheduler": trainer.scheduler}
    start = 0
    path = os.path.join(out_dir, "model.pth")
    if os.path.exists(path):                         # resume (load_checkpoint of the reference trainer)
        ngp.install_pickle_shims()
        snap = torch.load(path, map_location=device, weights_only=False)
        field.load_state_dict(snap["model"])
        grid.load_state_dict(snap["occupancy_grid"])
        if not config.no_load_opt and "optimizer" in snap:
            trainer.optimizer.load_state_dict(snap["optimizer"])
        if not config.no_load_scheduler and "scheduler" in snap:
            trainer.scheduler.load_state_dict(snap["scheduler"])
        start = int(snap.get("step", 0)) + 1
    score, t0 = 0.0, time.time()
    for it in range(start, config.max_iterations + 1):
        loss = trainer.step(it)
        if it % config.n_validation == 0 and it > 0:
            score = validate(trainer, val_set, out_dir)
            print(f"{out_dir}: step {it} loss {loss} val psnr {score:.2f} ({time.time() - t0:.1f} s)", flush=True)
        if it % config.n_checkpoint == 0 and it > 0 or it == config.max_iterations:
            ckpt.save(models, optims, it, scheds, meta, score=score)
    return score


def train(config, device):
    n_blocks = random.randint(config.min_num_blocks, config.max_num_blocks) if config.multi_blocks else 1
    train_sets = SubjectImages.load(config.dataset, config.root_dir, config.scene, "train", device, config.multi_blocks, n_blocks)
    val_sets = SubjectImages.load(config.dataset, config.root_dir, config.scene, "test", device, config.multi_blocks, n_blocks)
    base = os.path.join(config.root_dir, "out", config.expname)
    scores = []
    for k, (tr, va) in enumerate(zip(train_sets, val_sets)):
        out_dir = os.path.join(base, f"block_{k}") if config.multi_blocks else base
        scores.append(train_block(config, tr, va, out_dir, device))
    return scores


def main(argv=None):
    config = config_parser(argv)
    if config.unbounded:
        raise NotImplementedError("train_ngp_nerf.py: unbounded scenes (contracted fields) are not supported")
    assert config.data_split_json != "" or config.scene != ""
    device = torch.device("cuda:0")
    if config.data_split_json != "" and config.scene == "":
        with open(config.data_split_json) as fp:
            scenes = list(json.load(fp).values())
        for scene in scenes:
            if not os.path.exists(os.path.join(config.root_dir, scene)):
                continue
            local = copy.deepcopy(config)
            local.scene, local.expname = scene, scene
            train(local, device)
    else:
        train(config, device)


if __name__ == "__main__":
    main()
