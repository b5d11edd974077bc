"""A registered SCENE of K NeRF blocks (1 <= K <= 4) as ONE voxel grid in the format of a block's voxel_grid.pt / voxel_mask.pt: the fused kernel of
csrc/scene_grid.hip (one launch: sample positions, the scene density of scene_field.SceneField, alpha / keep, the blended 18-direction mean colour,
the [X,Y,Z,7] rows).  The registration network reads nothing but such grids, so a registered scene written here is again one of its inputs.  Rule,
kernel and measurements: DESIGN.md §3l; CPU restatement: tests/scene_grid_restatement.py."""
import json
import os
from typing import Optional

import torch

from . import ngp
from .scene_field import SceneField, scene_box          # noqa: F401  (scene_box: the box of the moved model aabbs, rounded outward to fp32)


def extract_grid(sf: SceneField, resolution=128, aabb=None, jitter=None, density_thre: float = 0.7, delta: float = 1e-2, surface: bool = False) -> dict:
    """SceneField.extract_grid: {"voxel_grid" [rx,ry,rz,7], "keep" bool [rx,ry,rz], "sigma", "voxel_mask" int64 ascending, "aabb"}."""
    return sf.extract_grid(resolution, aabb, jitter, density_thre, delta, surface)


def kept_iou(mask_a: torch.Tensor, mask_b: torch.Tensor, n_cells: int) -> float:
    """Intersection over union of two sets of flat cell indices of the same grid (1.0 when both are empty)."""
    a = torch.zeros(n_cells, dtype=torch.bool, device=mask_a.device)
    b = torch.zeros_like(a)
    a[mask_a] = True
    b[mask_b] = True
    union = int((a | b).sum())
    return 1.0 if union == 0 else int((a & b).sum()) / union


def registered_scene_grid(output_dir: str, scene, G_gt, G_sync, dataset: str, device, resolution=128, density_thre: float = 0.7,
                          power: float = 4.0, jitter_seed: Optional[int] = 0) -> dict:
    """eval_nerf_regtr.py --scene_voxel_grid for one scene: ALL its blocks as one voxel grid per pose set, in the anchor's frame, written through
    ngp.save_voxel_grid in the files of a block's extraction — scene_voxel_grid_{gt,aligned}.pt / scene_voxel_mask_{gt,aligned}.pt (surface AND
    density mask: what the registration dataset reads) and scene_density_voxel_grid_* / scene_density_voxel_mask_* (density mask only), each with
    the kept samples as scene_*_point_cloud_{gt,aligned}.ply — and scene_voxel_grid.json with K, the resolution, the box, the kept cells per pose
    set and the IoU of the two kept sets.  Both pose sets use the SAME box (scene_box under the ground-truth poses) and the same jitter
    (torch.rand of jitter_seed on the host; None: the cell centres), so the IoU is a geometric score of the synchronised poses.  The blocks are
    loaded, the camera centroids taken from the checkpoints' camera_poses and every block given its G_b as registered_scene_mesh does; the surface
    mask needs the checkpoints' render_step_size (without it every density-kept cell stays); `dataset` is accepted for the same signature."""
    from .render import load_render_block
    loaded = [load_render_block(b["nerf_path"], device) for b in scene]
    centers = [torch.as_tensor(m["camera_poses"]).float()[:, :3, 3].mean(0).cpu() for _, _, m in loaded]
    metas = [m for _, _, m in loaded]
    surface = all("camera_poses" in m and m.get("render_step_size") is not None for m in metas)
    G_gt, G_sync = torch.as_tensor(G_gt).double().cpu(), torch.as_tensor(G_sync).double().cpu()
    os.makedirs(output_dir, exist_ok=True)
    res = (int(resolution),) * 3 if isinstance(resolution, int) else tuple(int(v) for v in resolution)
    n = res[0] * res[1] * res[2]
    jitter = None
    if jitter_seed is not None:
        jitter = torch.rand(n, 3, generator=torch.Generator().manual_seed(int(jitter_seed))).to(device)
    box = scene_box([f._aabb_host() for f, _, _ in loaded], [G_gt[b] for b in range(len(loaded))])
    out, stats = {}, {"K": len(loaded), "resolution": list(res), "aabb": box, "density_thre": float(density_thre), "power": float(power),
                      "surface": bool(surface)}
    for name, G in (("gt", G_gt), ("aligned", G_sync)):
        sf = SceneField([(f, g, centers[b], G[b]) for b, (f, g, _) in enumerate(loaded)], power=power, metas=metas)
        dens = sf.extract_grid(res, box, jitter, density_thre)
        both = sf.extract_grid(res, box, jitter, density_thre, surface=True) if surface else dens
        for kind, e in (("voxel", both), ("density_voxel", dens)):
            rows = e["voxel_grid"].reshape(-1, 7)[e["voxel_mask"]]
            ngp.save_voxel_grid(output_dir, e["voxel_grid"], e["voxel_mask"], prefix=f"scene_{kind}", points=rows[:, :3], colors=rows[:, 3:6])
            for part, ext in (("grid", "pt"), ("mask", "pt"), ("point_cloud", "ply")):
                os.replace(os.path.join(output_dir, f"scene_{kind}_{part}.{ext}"), os.path.join(output_dir, f"scene_{kind}_{part}_{name}.{ext}"))
        stats[name] = {"kept": int(both["voxel_mask"].numel()), "kept_density": int(dens["voxel_mask"].numel())}
        out[name] = {"voxel": both, "density_voxel": dens}
    stats["iou"] = kept_iou(out["gt"]["voxel"]["voxel_mask"], out["aligned"]["voxel"]["voxel_mask"], n)
    stats["iou_density"] = kept_iou(out["gt"]["density_voxel"]["voxel_mask"], out["aligned"]["density_voxel"]["voxel_mask"], n)
    with open(os.path.join(output_dir, "scene_voxel_grid.json"), "w") as f:
        json.dump(stats, f, indent=2)
    out["stats"] = stats
    return out
