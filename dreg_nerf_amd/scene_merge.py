"""A registered SCENE of K NeRF blocks merged into ONE NeRF block by field distillation: a fresh Instant-NGP field is trained on
points to reproduce the scene's radiance — density from scene_field.SceneField, colour blended by §3l's rule —, and written as a model.pth that
every single-block consumer accepts with no knowledge of poses or K.  A composition of existing calls over the point-wise backward of
csrc/field_train.hip (field_train.field_points); no kernel of its own.

  scene_radiance           the teacher: (sigma, rgb) of the scene at scene-frame points seen along scene-frame directions
  SceneDistiller           the student, its sampler, loss and step
  merge_registered_scene   eval_nerf_regtr.py --merge_scene for one scene"""
import json
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import field_train, ngp, ngp_train
from .scene_field import SceneField, scene_box


def dirs_to_frame(Rf, d: torch.Tensor) -> torch.Tensor:
    """Directions d [N,3] fp32 of the scene frame in the frame of a block with the fp32 rotation Rf (block -> scene): R^T d by the elementwise
    fp32 expression scene_field.points_to_frame uses for positions."""
    return torch.stack([(float(Rf[0, k]) * d[:, 0] + float(Rf[1, k]) * d[:, 1]) + float(Rf[2, k]) * d[:, 2] for k in range(3)], dim=1)


def blend_colors(a, colors):
    """§3l's colour rule over K blocks: a a list of K [N] fp32 (a_b = omega_b sigma_b), colors a list of K [N,3] fp32 or None (a block nothing
    carries).  rgb = (sum_b fl(a_b c_b)) / (sum_b a_b), both sums in block order; exactly one block with a_b != 0: that block's colour bit for
    bit; the denominator or a product not finite: the colour of the block with the largest a_b (lowest index on a tie); no carrier: 0."""
    K = len(a)
    zero3 = torch.zeros(a[0].shape[0], 3, dtype=torch.float32, device=a[0].device)
    cols = [zero3 if c is None else c for c in colors]
    den = a[0]
    prods = [a[0][:, None] * cols[0]]
    num = prods[0]
    for b in range(1, K):
        den = den + a[b]
        prods.append(a[b][:, None] * cols[b])
        num = num + prods[b]
    carriers = sum((a[b] != 0).to(torch.int32) for b in range(K))
    finite = torch.isfinite(den)
    for p in prods:
        finite = finite & torch.isfinite(p).all(dim=1)
    mix = num / torch.where(den != 0, den, torch.ones_like(den))[:, None]
    best, best_a = cols[0], a[0]
    for b in range(1, K):
        take = a[b] > best_a                                  # strictly larger: the lowest index wins a tie
        best = torch.where(take[:, None], cols[b], best)
        best_a = torch.where(take, a[b], best_a)
    mix = torch.where(finite[:, None], mix, best)
    for b in range(K):
        mix = torch.where(((a[b] != 0) & (carriers == 1))[:, None], cols[b], mix)
    return torch.where((carriers > 0)[:, None], mix, zero3)


@torch.no_grad()
def scene_radiance(sf: SceneField, x: torch.Tensor, dirs: torch.Tensor):
    """(sigma [N], rgb [N,3]) of the registered scene at the scene-frame points x [N,3] seen along the scene-frame unit directions dirs [N,3]:
    sigma = SceneField.query(x); per block with some a_b = omega_b sigma_b != 0 the block's own colour query_rgb(d_b, query_raw(x_b)) at
    x_b = points_to_block(b, x), d_b = R_b^T d (x and d untouched where the block has no pose), blended by blend_colors."""
    x = x.reshape(-1, 3).to(sf.device).float().contiguous()
    dirs = dirs.reshape(-1, 3).to(sf.device).float().contiguous()
    sigma, w, sb = sf.query(x, parts=True)
    a = [w[:, b] * sb[:, b] for b in range(sf.K)]
    colors = []
    for b, field in enumerate(sf.fields):
        if not bool((a[b] != 0).any()):
            colors.append(None)
            continue
        xb = sf.points_to_block(b, x).contiguous()
        db = dirs if sf.R[b] is None else dirs_to_frame(sf.R[b], dirs).contiguous()
        colors.append(field.query_rgb(db, field.query_raw(xb)[1][:, 1:].float()).float())
    return sigma, blend_colors(a, colors)


def distill_loss(sigma_s, rgb_s, sigma_t, rgb_t):
    """mean((log1p sigma_s - log1p sigma_t)^2) + smooth_l1(rgb_s[m], rgb_t[m]) over m = sigma_t > 0 (the colour term is dropped when m is empty)."""
    loss = ((torch.log1p(sigma_s) - torch.log1p(sigma_t)) ** 2).mean()
    m = sigma_t > 0
    if bool(m.any()):
        loss = loss + F.smooth_l1_loss(rgb_s[m], rgb_t[m])
    return loss


def sample_points(aabb, keep_idx: torch.Tensor, res, n_points: int, gen: torch.Generator, device):
    """n_points points in the aabb and as many unit directions, all from `gen`: half uniform in the aabb, half in uniformly drawn cells of
    keep_idx (flat indices of a res = (rx, ry, rz) grid over the aabb, z fastest) with a uniform offset inside the cell; all uniform when no cell
    is kept.  Directions: normalised Gaussians."""
    lo = torch.tensor(aabb[:3], dtype=torch.float32, device=device)
    ext = torch.tensor(aabb[3:], dtype=torch.float32, device=device) - lo
    u = torch.rand(n_points, 3, generator=gen, device=device)
    n_cells = n_points // 2 if keep_idx.numel() else 0
    if n_cells:
        pick = keep_idx[torch.randint(keep_idx.numel(), (n_cells,), generator=gen, device=device)]
        rx, ry, rz = res
        cell = torch.stack([pick // (ry * rz), (pick // rz) % ry, pick % rz], dim=1).float()
        u[:n_cells] = ((cell + u[:n_cells]) / torch.tensor([rx, ry, rz], dtype=torch.float32, device=device)).clamp(0.0, 1.0)
    x = lo + u * ext
    d = F.normalize(torch.randn(n_points, 3, generator=gen, device=device), dim=-1)
    return x, d


class SceneDistiller:
    """Distils sf (a SceneField) into a fresh NGPradianceField over `aabb` (default sf.box()).  Every default — the point count, the step count,
    the 50/50 sampling, the loss and its unit weights, lr and schedule — is untuned."""

    def __init__(self, sf: SceneField, aabb=None, n_points: int = 1 << 16, max_iterations: int = 2000, seed: int = 0, grid_resolution: int = 128):
        self.sf, self.device = sf, sf.device
        self.aabb = [float(v) for v in (sf.box() if aabb is None else (aabb.tolist() if torch.is_tensor(aabb) else aabb))]
        self.n_points, self.max_iterations = int(n_points), int(max_iterations)
        self.field = ngp.NGPradianceField(self.aabb).to(self.device)
        self.grid = ngp.OccupancyGrid(self.aabb, int(grid_resolution)).to(self.device)
        self.render_step_size = ngp_train.render_step_size_of(self.aabb)
        self.optimizer = ngp_train.NGPAdam(self.field, lr=1e-2, eps=1e-15)
        self.scheduler = ngp_train.multistep_lr(self.optimizer, self.max_iterations)
        self.gen = torch.Generator(device=self.device).manual_seed(int(seed))
        self.res = (int(grid_resolution),) * 3
        self.keep_idx = sf.extract_grid(self.res, self.aabb, density_thre=0.0)["voxel_mask"]
        self.last = {}

    def occ_eval_fn(self, x):
        return self.field.query_density(x) * self.render_step_size

    def sample(self):
        return sample_points(self.aabb, self.keep_idx, self.res, self.n_points, self.gen, self.device)

    def step(self, it: int) -> float:
        self.field.train()
        self.grid.train()
        self.grid.every_n_step(step=it, occ_eval_fn=self.occ_eval_fn, occ_thre=1e-2)
        x, d = self.sample()
        sigma_t, rgb_t = scene_radiance(self.sf, x, d)
        with torch.enable_grad():                              # (the evaluator calls this under no_grad)
            sigma_s, rgb_s = field_train.field_points(self.field, x, d)
            loss = distill_loss(sigma_s, rgb_s, sigma_t, rgb_t)
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
        self.optimizer.step()
        self.scheduler.step()
        self.last = {"loss": float(loss.detach()), "step": it}
        return self.last["loss"]

    def run(self, log=None):
        for it in range(self.max_iterations):
            loss = self.step(it)
            if log is not None and (it % 100 == 0 or it == self.max_iterations - 1):
                log(f"distill step {it}: loss {loss:.5f}")
        self.grid._update(0, self.occ_eval_fn, occ_thre=1e-2)             # step 0 < warm-up: every cell is refreshed once
        self.field.eval()
        return self.last.get("loss")

    def meta(self, camera_poses) -> dict:
        """The meta data of a train_ngp_nerf.py checkpoint for the merged block (no block_id)."""
        return {"aabb": list(self.aabb), "unbounded": False, "grid_resolution": int(self.res[0]), "contraction_type": ngp.ContractionType.AABB,
                "near_plane": None, "far_plane": None, "render_step_size": self.render_step_size, "alpha_thre": 0.0, "cone_angle": 0.0,
                "camera_poses": camera_poses}

    def save(self, out_dir: str, camera_poses):
        from .checkpoint import CheckPointManager
        ckpt = CheckPointManager(save_path=out_dir, max_to_keep=1, verbose=False)
        ckpt.save({"model": self.field, "occupancy_grid": self.grid}, {"optimizer": self.optimizer}, self.max_iterations, {"scheduler": self.scheduler},
                  self.meta(camera_poses), score=0.0)
        return os.path.join(out_dir, "model.pth")


def merge_registered_scene(output_dir: str, scene, G_gt, G_sync, dataset: str, device, max_iterations: int = 2000, n_points: int = 1 << 16,
                           power: float = 4.0, seed: int = 0, n_views: int = 4, log=None) -> dict:
    """eval_nerf_regtr.py --merge_scene for one scene: ALL its blocks distilled into one NeRF block per pose set — merged_block_gt/model.pth under
    the ground-truth G, merged_block_aligned/model.pth under the synchronised G, both over the SAME box (scene_box under the ground-truth poses),
    with every key train_ngp_nerf.py writes; camera_poses = all blocks' cameras moved by their G_b, no block_id — and merged_block.json: K, steps,
    points, the final loss, and PSNR / SSIM (image_metrics) between render_image of the merged block and render_scene_image of the K blocks from
    up to n_views of the scene's cameras.  The blocks are loaded and posed as scene_grid.registered_scene_grid does."""
    from . import render as R
    loaded = [R.load_render_block(b["nerf_path"], device) for b in scene]
    centers = [torch.as_tensor(m["camera_poses"]).float()[:, :3, 3].mean(0).cpu() for _, _, m in loaded]
    G_gt, G_sync = torch.as_tensor(G_gt).double().cpu(), torch.as_tensor(G_sync).double().cpu()
    os.makedirs(output_dir, exist_ok=True)
    box = scene_box([f._aabb_host() for f, _, _ in loaded], [G_gt[b] for b in range(len(loaded))])
    Kc, W, H = R.intrinsics(dataset)
    out, stats = {}, {"K": len(loaded), "steps": int(max_iterations), "points": int(n_points), "aabb": box, "power": float(power)}
    for name, G in (("gt", G_gt), ("aligned", G_sync)):
        sf = SceneField([(f, g, centers[b], G[b]) for b, (f, g, _) in enumerate(loaded)], power=power)
        dist = SceneDistiller(sf, box, n_points, max_iterations, seed)
        loss = dist.run(log)
        cams = torch.cat([(G[b] @ torch.as_tensor(m["camera_poses"]).double().cpu()).float() for b, (_, _, m) in enumerate(loaded)], dim=0)
        path = dist.save(os.path.join(output_dir, f"merged_block_{name}"), cams)
        pick = cams[torch.linspace(0, cams.shape[0] - 1, min(int(n_views), cams.shape[0])).round().long()]
        merged, _ = R.render_views(dist.field, dist.grid, dict(dist.meta(cams), aabb_host=list(dist.aabb)), pick, Kc, W, H)
        teacher = R.render_blocks_views(loaded, G, pick, Kc, W, H)[0]
        psnr, ssim = R._stack_metrics([torch.from_numpy(v).to(teacher[0].device) for v in merged], teacher)
        stats[name] = {"final_loss": loss, "psnr": [float(v) for v in psnr], "ssim": [float(v) for v in ssim], "model": path,
                       "occupied_cells": int(dist.grid.binary.sum())}
        out[name] = dist
    with open(os.path.join(output_dir, "merged_block.json"), "w") as f:
        json.dump(stats, f, indent=2)
    out["stats"] = stats
    return out
