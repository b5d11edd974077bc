"""Volume rendering of a NeRF block through the fused kernel of csrc/render.hip: the reference's render_image
(conerf/utils/utils.py:44-141, nerfacc 0.3.5 ray_marching + rendering) with no sample list, plus the pixel rays of
NeRFPoseOnlyDataset (conerf/datasets/register/nerf_pose_only_dataset.py:56-152) and the views eval_nerf_regtr.py --render_views writes
(render_videos, eval_nerf_regtr.py:113-172 and :345-369 of the reference).

The marching / compositing rule is stated in csrc/render.hip and DESIGN.md ("Volume renderer"); nerfacc is absent from the reference tree,
so parity is unpinned and that rule is the specification (CPU restatement: tests/render_restatement.py).

A registered pair of blocks as ONE scene goes through the fused two-block kernel of csrc/render_pair.hip (rays_to_block, render_pair_image,
render_pair_views, and render_scene_merged for eval_nerf_regtr.py --render_merged; rule: DESIGN.md §3e, CPU restatement:
tests/render_pair_restatement.py).

Up to four registered blocks as ONE scene go through the fused K-block kernel of csrc/render_scene.hip (render_scene_image, render_blocks_views;
rule: DESIGN.md §3j, CPU restatement: tests/render_scene_restatement.py); with two blocks it is the pair kernel bit for bit."""
import collections
import ctypes
import math
import os
import shutil
import subprocess
from typing import Optional

import numpy as np
import torch

from . import lib as L
from . import ngp
from . import visibility

Rays = collections.namedtuple("Rays", ("origins", "viewdirs"))

# Camera intrinsics of the registration datasets (NeRFPoseOnlyDataset.load_data): (width, height, fx, fy, cx, cy), OpenGL cameras.
_FX_800 = 0.5 * 800 / math.tan(0.5 * 0.6911112070083618)          # camera_angle_x of the Blender-style renders
INTRINSICS = {
    "objaverse": (800, 800, _FX_800, _FX_800, 400.0, 400.0),
    "nerf_synthetic": (800, 800, _FX_800, _FX_800, 400.0, 400.0),
    "scannerf": (1440, 1080, 1522.1201085541113, 1521.954743529035, 727.9348613007779, 541.5426465751151),
}


def intrinsics(dataset: str):
    """(K fp32 [3,3], width, height) of a dataset's cameras."""
    if dataset not in INTRINSICS:
        raise NotImplementedError(f"no camera intrinsics for dataset {dataset!r} (known: {sorted(INTRINSICS)})")
    w, h, fx, fy, cx, cy = INTRINSICS[dataset]
    return torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float32), w, h


def pixel_rays(c2w: torch.Tensor, K: torch.Tensor, W: int, H: int, opengl: bool = True) -> Rays:
    """Rays through the pixel centres of one camera (NeRFPoseOnlyDataset.fetch_data): c2w [3,4] or [4,4] -> Rays of [H,W,3] origins and unit
    viewdirs.  Pixel (x, y) looks along ((x - cx + 0.5) / fx, (y - cy + 0.5) / fy, 1), with y and z negated for OpenGL cameras."""
    c2w = c2w.float()
    K = K.to(c2w.device).float()
    x, y = torch.meshgrid(torch.arange(W, device=c2w.device), torch.arange(H, device=c2w.device), indexing="xy")
    x, y = x.flatten(), y.flatten()
    s = -1.0 if opengl else 1.0
    cam = torch.nn.functional.pad(torch.stack([(x - K[0, 2] + 0.5) / K[0, 0], (y - K[1, 2] + 0.5) / K[1, 1] * s], dim=-1), (0, 1), value=s)
    directions = (cam[:, None, :] * c2w[None, :3, :3]).sum(dim=-1)
    origins = torch.broadcast_to(c2w[:3, -1], directions.shape)
    viewdirs = directions / torch.linalg.norm(directions, dim=-1, keepdim=True)
    return Rays(origins.reshape(H, W, 3), viewdirs.reshape(H, W, 3))


class BlockGrid:
    """The occupancy grid of a loaded block as render_image reads it (roi_aabb, binary, contraction_type), with the uint8 copy and the coarse bits
    the kernel walks (visibility.load_block's meta)."""

    def __init__(self, roi_aabb, binary_u8: torch.Tensor, coarse_bits: Optional[torch.Tensor] = None, contraction_type=ngp.ContractionType.AABB):
        self.roi_aabb = [float(v) for v in (roi_aabb.tolist() if torch.is_tensor(roi_aabb) else roi_aabb)]
        self.binary_u8 = binary_u8 if binary_u8.dtype == torch.uint8 else binary_u8.to(torch.uint8)
        self.binary_u8 = self.binary_u8.contiguous()
        self.coarse_bits = coarse_bits
        self.contraction_type = contraction_type

    @property
    def binary(self):
        return self.binary_u8.view(torch.bool)


def _grid_parts(occupancy_grid, dev):
    """(roi aabb as 6 host floats, uint8 occupancy on the device, coarse bits) of a BlockGrid or an ngp.OccupancyGrid."""
    if getattr(getattr(occupancy_grid, "contraction_type", None), "name", "AABB") != "AABB":
        raise NotImplementedError("render_image: only ContractionType.AABB occupancy grids are rendered (DESIGN.md: no contraction)")
    if isinstance(occupancy_grid, BlockGrid):
        b8, bits = occupancy_grid.binary_u8, occupancy_grid.coarse_bits
        roi = occupancy_grid.roi_aabb
    else:
        b = occupancy_grid.binary.to(dev)
        b8 = (b.contiguous().view(torch.uint8) if b.dtype == torch.bool else (b != 0).to(torch.uint8)).contiguous()
        bits = None
        roi = [float(v) for v in occupancy_grid.roi_aabb.tolist()]
    if bits is None:
        bits = visibility.coarse_occupancy_bits(b8)
    return roi, b8, bits


def render_image(radiance_field, occupancy_grid, rays, scene_aabb, near_plane: Optional[float] = None, far_plane: Optional[float] = None,
                 render_step_size: float = 1e-3, render_bkgd: Optional[torch.Tensor] = None, cone_angle: float = 0.0, alpha_thre: float = 0.0,
                 test_chunk_size: int = 8192):
    """The reference's render_image (inference): rays with origins / viewdirs shaped [N,3] or [H,W,3] -> (colors [...,3], opacities [...,1],
    depths [...,1], n_rendering_samples: int).  One launch of the fused kernel for all rays: test_chunk_size is accepted and has no effect (there
    is no sample list to bound).  Not differentiable: raises when gradients are requested."""
    if radiance_field.training or rays.origins.requires_grad or rays.viewdirs.requires_grad:
        raise RuntimeError("render_image: the fused renderer is inference only (no backward); call it under torch.no_grad() with an eval-mode field")
    if cone_angle != 0.0:
        raise NotImplementedError("render_image: cone_angle != 0 (unbounded marching) is not supported")
    if scene_aabb is None or getattr(radiance_field, "unbounded", False):
        raise NotImplementedError("render_image: unbounded scenes (no scene aabb / contracted field) are not supported")
    with torch.no_grad():
        return _render(radiance_field, occupancy_grid, rays, scene_aabb, near_plane, far_plane, render_step_size, render_bkgd, alpha_thre)


def _render(field, occupancy_grid, rays, scene_aabb, near_plane, far_plane, render_step_size, render_bkgd, alpha_thre):
    lib = L.load()
    shp = rays.origins.shape
    base16, col16 = field._prepared()
    dev = base16.device
    o = rays.origins.reshape(-1, 3).to(dev).float().contiguous()
    d = rays.viewdirs.reshape(-1, 3).to(dev).float().contiguous()
    n = o.shape[0]
    roi, b8, bits = _grid_parts(occupancy_grid, dev)
    bk = [0.0, 0.0, 0.0] if render_bkgd is None else [float(v) for v in torch.as_tensor(render_bkgd).reshape(-1).tolist()]
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    opacity = torch.empty(n, dtype=torch.float32, device=dev)
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)          # surviving samples, then the ray queue
    visibility.OVERRUN.check()
    L.check(lib.dreg_ngp_render(L.ptr(o), L.ptr(d), n, L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], L.ptr(bits),
                                *field.density_ptrs(), *field.color_ptrs(),
                                *field._levels, L.f6(roi), L.f6(scene_aabb), L.f6(field._aabb_host()),
                                -math.inf if near_plane is None else float(near_plane), math.inf if far_plane is None else float(far_plane),
                                float(render_step_size), float(alpha_thre or 0.0), 1e-4, L.f3(bk),
                                L.ptr(rgb), L.ptr(opacity), L.ptr(depth), counters.data_ptr(), counters.data_ptr() + 8, L.stream()),
            "dreg_ngp_render")
    visibility.OVERRUN.watch(counters[1:])
    n_samples = int(counters[0].item())
    visibility.OVERRUN.check(wait=True)
    return rgb.view(*shp[:-1], 3), opacity.view(*shp[:-1], 1), depth.view(*shp[:-1], 1), n_samples


# ---------------------------------------------------------------------------------------------------------------- a registered pair as one scene
def _pose44(pose: torch.Tensor) -> torch.Tensor:
    """A [3,4] or [4,4] pose as fp64 [4,4] on the host."""
    P = pose.detach().double().cpu().reshape(-1, 4)
    if P.shape[0] == 3:
        P = torch.cat([P, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)])
    if P.shape != (4, 4):
        raise ValueError(f"pose must be [3,4] or [4,4], got {tuple(pose.shape)}")
    return P


def rays_to_block(rays: Rays, pose: torch.Tensor) -> Rays:
    """Rays given in the frame `pose` = [R|t] maps TO, expressed in the frame it maps FROM (target-frame rays for the source block of a registered
    pair): o' = R^T (o - t), d' = R^T d / |R^T d|, formed in fp64 and rounded to fp32.  pose: [3,4] or [4,4]; shapes are kept."""
    P = _pose44(pose).to(rays.origins.device)
    Rm, t = P[:3, :3], P[:3, 3]
    o = (rays.origins.double() - t) @ Rm                       # row vectors: (R^T v)^T = v^T R
    d = rays.viewdirs.double() @ Rm
    d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    return Rays(o.float(), d.float())


PAIR_OPTS = ("scene_aabb", "near_plane", "far_plane", "render_step_size", "alpha_thre", "cone_angle")


def _pair_block_args(field, grid, rays, opts, center, dev, keep):
    """One block's arguments of dreg_ngp_render_pair (the C ABI's order); the tensors and ctypes arrays they point into are appended to `keep`."""
    base16, col16 = field._prepared()
    o = rays.origins.reshape(-1, 3).to(dev).float().contiguous()
    d = rays.viewdirs.reshape(-1, 3).to(dev).float().contiguous()
    roi, b8, bits = _grid_parts(grid, dev)
    near, far = opts.get("near_plane"), opts.get("far_plane")
    arrs = [L.f6(roi), L.f6(opts["scene_aabb"]), L.f6(field._aabb_host()), L.f3(torch.as_tensor(center))]
    keep.extend([o, d, b8, bits, base16, col16] + arrs)
    return [L.ptr(o), L.ptr(d), L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], L.ptr(bits),
            *field.density_ptrs(), *field.color_ptrs(), *field._levels, arrs[0], arrs[1], arrs[2],
            -math.inf if near is None else float(near), math.inf if far is None else float(far),
            float(opts.get("render_step_size", 1e-3)), float(opts.get("alpha_thre") or 0.0), arrs[3]]


def render_pair_image(src_field, src_grid, tgt_field, tgt_grid, rays, pose, src_opts, tgt_opts, src_center, tgt_center, power: float = 4.0,
                      render_bkgd: Optional[torch.Tensor] = None):
    """A registered pair of blocks rendered as ONE scene by the fused two-block kernel (csrc/render_pair.hip): rays with origins /
    viewdirs shaped [N,3] or [H,W,3] in the TARGET frame, pose = [R|t] ([3,4] or [4,4]) mapping the source frame to the target frame ->
    (colors [...,3], opacities [...,1], depths [...,1], weight_src [...,1], n_rendering_samples: int); weight_src is the part of the opacity that
    source samples contributed.  *_opts: dicts with scene_aabb, near_plane, far_plane, render_step_size, alpha_thre (of that block's training);
    *_center: the centroid of the block's cameras in its own frame; power: the exponent of the overlap weight.  Inference only."""
    for f in (src_field, tgt_field):
        if f.training:
            raise RuntimeError("render_pair_image: the fused renderer is inference only (no backward); call it under torch.no_grad() with eval-mode fields")
    if rays.origins.requires_grad or rays.viewdirs.requires_grad:
        raise RuntimeError("render_pair_image: the fused renderer is inference only (no backward); call it under torch.no_grad() with eval-mode fields")
    for f, opts in ((src_field, src_opts), (tgt_field, tgt_opts)):
        unknown = set(opts) - set(PAIR_OPTS)
        if unknown:
            raise TypeError(f"render_pair_image: unknown options {sorted(unknown)} (known: {PAIR_OPTS})")
        if float(opts.get("cone_angle") or 0.0) != 0.0:
            raise NotImplementedError("render_pair_image: cone_angle != 0 (unbounded marching) is not supported")
        if opts.get("scene_aabb") is None or getattr(f, "unbounded", False):
            raise NotImplementedError("render_pair_image: unbounded scenes (no scene aabb / contracted field) are not supported")
    with torch.no_grad():
        lib = L.load()
        shp = rays.origins.shape
        dev = tgt_field._prepared()[0].device
        if src_field._prepared()[0].device != dev:
            raise ValueError("render_pair_image: both blocks must be on the same device")
        keep = []
        src_args = _pair_block_args(src_field, src_grid, rays_to_block(rays, pose), src_opts, src_center, dev, keep)
        tgt_args = _pair_block_args(tgt_field, tgt_grid, rays, tgt_opts, tgt_center, dev, keep)
        n = rays.origins.reshape(-1, 3).shape[0]
        bk = [0.0, 0.0, 0.0] if render_bkgd is None else [float(v) for v in torch.as_tensor(render_bkgd).reshape(-1).tolist()]
        rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
        opacity, depth, wsrc = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        counters = torch.zeros(2, dtype=torch.int64, device=dev)          # surviving samples, then the ray queue
        visibility.OVERRUN.check()
        L.check(lib.dreg_ngp_render_pair(n, *src_args, *tgt_args, float(power), 1e-4, L.f3(bk),
                                         L.ptr(rgb), L.ptr(opacity), L.ptr(depth), L.ptr(wsrc), counters.data_ptr(), counters.data_ptr() + 8, L.stream()),
                "dreg_ngp_render_pair")
        visibility.OVERRUN.watch(counters[1:])
        n_samples = int(counters[0].item())
        visibility.OVERRUN.check(wait=True)
        return rgb.view(*shp[:-1], 3), opacity.view(*shp[:-1], 1), depth.view(*shp[:-1], 1), wsrc.view(*shp[:-1], 1), n_samples


def block_pair_opts(meta) -> dict:
    """The options render_pair_image takes for one block, from load_render_block's meta (what render_views passes to render_image)."""
    return dict(scene_aabb=meta["aabb_host"], near_plane=meta.get("near_plane"), far_plane=meta.get("far_plane"),
                render_step_size=float(meta["render_step_size"]), alpha_thre=float(meta.get("alpha_thre") or 0.0),
                cone_angle=float(meta.get("cone_angle") or 0.0))


def render_pair_views(blocks, pose: torch.Tensor, poses_c2w: torch.Tensor, K: torch.Tensor, W: int, H: int, bkgd=(1.0, 1.0, 1.0)):
    """render_views for a registered pair: blocks = ((field, grid, meta) of the source, of the target), pose maps the source frame to the target
    frame, poses_c2w [N,4,4] are cameras in the TARGET frame.  The blocks' camera centroids come from meta["camera_poses"].  Returns lists of
    device tensors: rgb [H,W,3], depth [H,W,1], weight_src [H,W,1]."""
    (sf, sg, sm), (tf, tg, tm) = blocks
    dev = tf._prepared()[0].device
    bk = torch.tensor(bkgd, dtype=torch.float32)
    centers = [torch.as_tensor(m["camera_poses"]).float()[:, :3, 3].mean(0).cpu() for m in (sm, tm)]
    so, to = block_pair_opts(sm), block_pair_opts(tm)
    rgbs, depths, shares = [], [], []
    for c2w in poses_c2w:
        rays = pixel_rays(c2w.to(dev), K, W, H)
        rgb, _, depth, wsrc, _ = render_pair_image(sf, sg, tf, tg, rays, pose, so, to, centers[0], centers[1], render_bkgd=bk)
        rgbs.append(rgb)
        depths.append(depth)
        shares.append(wsrc)
    return rgbs, depths, shares


# ---------------------------------------------------------------------------------------------------------------- K registered blocks as one scene
def render_scene_image(blocks, rays, power: float = 4.0, render_bkgd: Optional[torch.Tensor] = None):
    """K registered blocks (1 <= K <= 4) rendered as ONE scene by the fused K-block kernel (csrc/render_scene.hip).
    blocks: a list of (field, grid, opts, center, pose) — opts as render_pair_image takes them (PAIR_OPTS), center the centroid of the block's
    cameras in its own frame, pose = G_b ([3,4] or [4,4]) mapping the block's frame to the frame the rays are given in (rays_to_block brings
    the rays into the block's frame), or None: the rays are passed to that block untouched (an identity pose would re-normalise the directions
    in fp64 and change their bits).  rays: origins / viewdirs shaped [N,3] or [H,W,3] -> (colors [...,3], opacities [...,1], depths [...,1],
    weight_block [...,K]: the part of the opacity each block's samples contributed, n_rendering_samples: int).  Inference only."""
    blocks = list(blocks)
    if not 1 <= len(blocks) <= L.SCENE_MAX_BLOCKS:
        raise ValueError(f"render_scene_image: {len(blocks)} blocks (1 to {L.SCENE_MAX_BLOCKS} are rendered as one scene)")
    if rays.origins.requires_grad or rays.viewdirs.requires_grad or any(b[0].training for b in blocks):
        raise RuntimeError("render_scene_image: the fused renderer is inference only (no backward); call it under torch.no_grad() with eval-mode fields")
    for f, _, opts, _, _ in blocks:
        unknown = set(opts) - set(PAIR_OPTS)
        if unknown:
            raise TypeError(f"render_scene_image: unknown options {sorted(unknown)} (known: {PAIR_OPTS})")
        if float(opts.get("cone_angle") or 0.0) != 0.0:
            raise NotImplementedError("render_scene_image: cone_angle != 0 (unbounded marching) is not supported")
        if opts.get("scene_aabb") is None or getattr(f, "unbounded", False):
            raise NotImplementedError("render_scene_image: unbounded scenes (no scene aabb / contracted field) are not supported")
    with torch.no_grad():
        lib = L.load()
        shp = rays.origins.shape
        dev = blocks[0][0].mlp_base.params.device                         # (asked of the parameters: _prepared() of a host field would launch on host memory)
        if any(b[0].mlp_base.params.device != dev for b in blocks[1:]):
            raise ValueError("render_scene_image: all blocks must be on the same device")
        keep = []
        arr = (L.SceneBlock * len(blocks))()
        names = [n for n, _ in L.SceneBlock._fields_]
        for i, (f, g, opts, center, pose) in enumerate(blocks):
            args = _pair_block_args(f, g, rays if pose is None else rays_to_block(rays, pose), opts, center, dev, keep)
            for name, v in zip(names, args):
                setattr(arr[i], name, ctypes.cast(v, ctypes.c_void_p) if isinstance(v, ctypes.Array) else v)
        n = rays.origins.reshape(-1, 3).shape[0]
        bk = [0.0, 0.0, 0.0] if render_bkgd is None else [float(v) for v in torch.as_tensor(render_bkgd).reshape(-1).tolist()]
        rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
        opacity, depth = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        wblock = torch.empty(n, len(blocks), dtype=torch.float32, device=dev)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)          # surviving samples, then the ray queue
        visibility.OVERRUN.check()
        L.check(lib.dreg_ngp_render_scene(n, len(blocks), ctypes.cast(arr, ctypes.c_void_p), float(power), 1e-4, L.f3(bk),
                                          L.ptr(rgb), L.ptr(opacity), L.ptr(depth), L.ptr(wblock), counters.data_ptr(), counters.data_ptr() + 8, L.stream()),
                "dreg_ngp_render_scene")
        visibility.OVERRUN.watch(counters[1:])
        n_samples = int(counters[0].item())
        visibility.OVERRUN.check(wait=True)
        return rgb.view(*shp[:-1], 3), opacity.view(*shp[:-1], 1), depth.view(*shp[:-1], 1), wblock.view(*shp[:-1], len(blocks)), n_samples


def render_blocks_views(blocks_loaded, poses, poses_c2w: torch.Tensor, K: torch.Tensor, W: int, H: int, bkgd=(1.0, 1.0, 1.0)):
    """render_pair_views for a registered scene of K blocks: blocks_loaded = [(field, grid, meta)] per block, poses = [G_b] mapping each block's
    frame to the common frame ([K,4,4] or a list), poses_c2w [N,4,4] cameras in the common frame.  The blocks' camera centroids come from
    meta["camera_poses"].  Returns lists of device tensors: rgb [H,W,3], depth [H,W,1], weight_block [H,W,K].
    (Not named render_scene_views: that is the --render_views writer of a pair, below.)"""
    dev = blocks_loaded[0][0]._prepared()[0].device
    bk = torch.tensor(bkgd, dtype=torch.float32)
    blocks = [(f, g, block_pair_opts(m), torch.as_tensor(m["camera_poses"]).float()[:, :3, 3].mean(0).cpu(), G)
              for (f, g, m), G in zip(blocks_loaded, poses)]
    rgbs, depths, shares = [], [], []
    for c2w in poses_c2w:
        rgb, _, depth, wb, _ = render_scene_image(blocks, pixel_rays(c2w.to(dev), K, W, H), render_bkgd=bk)
        rgbs.append(rgb)
        depths.append(depth)
        shares.append(wb)
    return rgbs, depths, shares


def load_render_block(path: str, device):
    """(field, BlockGrid, meta) of a NeRF block checkpoint for rendering, through visibility.load_block's cache (meta has near_plane / far_plane)."""
    field, _, meta = visibility.load_block(path, device)
    if getattr(meta["contraction_type"], "name", "AABB") != "AABB" or meta["unbounded"]:
        raise NotImplementedError("rendering needs an AABB-contracted, bounded block")
    return field, BlockGrid(meta["aabb_host"], meta["binary_u8"], meta["coarse_bits"]), meta


def render_views(field, grid, meta, poses: torch.Tensor, K: torch.Tensor, W: int, H: int, bkgd=(1.0, 1.0, 1.0)):
    """Render one block from every camera-to-world pose [N,4,4] (synthesize_novel_views of the reference, white background): lists of
    rgb [H,W,3] and depth [H,W,1] numpy arrays."""
    dev = field._prepared()[0].device
    bk = torch.tensor(bkgd, dtype=torch.float32)
    images, depths = [], []
    for c2w in poses:
        rays = pixel_rays(c2w.to(dev), K, W, H)
        rgb, _, depth, _ = render_image(field, grid, rays, meta["aabb_host"], near_plane=meta.get("near_plane"), far_plane=meta.get("far_plane"),
                                        render_step_size=float(meta["render_step_size"]), render_bkgd=bk, cone_angle=float(meta.get("cone_angle") or 0.0),
                                        alpha_thre=float(meta.get("alpha_thre") or 0.0))
        images.append(rgb.cpu().numpy())
        depths.append(depth.cpu().numpy())
    return images, depths


# ---------------------------------------------------------------------------------------------------------------- evaluator views
def pose_sets(src_cams: torch.Tensor, tgt_cams: torch.Tensor, pose_gt: torch.Tensor, pose_pred: torch.Tensor):
    """The three render sets of the reference's evaluator (eval_nerf_regtr.py:331-369): {prefix: (source-block poses, target-block poses)};
    pose_gt / pose_pred are [4,4] or [3,4].
    P maps the source frame to the target frame; the source block is rendered from its own cameras and the target's cameras brought into its
    frame (inv(P) @ tgt), the target block from the source cameras brought into its frame (P @ src) and its own."""
    src_cams, tgt_cams = src_cams.float().cpu(), tgt_cams.float().cpu()
    out = {}
    for prefix, P in (("gt", pose_gt), ("aligned", pose_pred)):
        P = P.detach().float().cpu().reshape(-1, 4)
        if P.shape[0] == 3:                                      # the model's [3,4] estimate
            P = torch.cat([P, torch.tensor([[0.0, 0.0, 0.0, 1.0]])])
        out[prefix] = (torch.cat([src_cams, torch.linalg.inv(P) @ tgt_cams], dim=0), torch.cat([P @ src_cams, tgt_cams], dim=0))
    both = torch.cat([src_cams, tgt_cams], dim=0)
    out["unaligned"] = (both, both.clone())
    return out


def colorize_depth(x: np.ndarray) -> np.ndarray:
    """colorize_np of the reference (conerf/utils/utils.py) without mask, range or colour bar: [H,W] -> [H,W,3] in [0,1], jet colour map over
    the percentiles (1, 100) of x (+1e-6 on the upper end)."""
    from matplotlib import colormaps
    vmin, vmax = np.percentile(x, (1, 100))
    vmax += 1e-6
    x = np.clip(x, vmin, vmax)
    x = (x - vmin) / (vmax - vmin)
    return colormaps["jet"](x)[:, :, :3]


def _png(path: str, img: np.ndarray):
    from PIL import Image
    Image.fromarray((np.clip(img, 0.0, 1.0) * 255).astype(np.uint8)).save(path)


def write_render_set(output_dir: str, prefix: str, src_rgbs, src_depths, tgt_rgbs, tgt_depths):
    """render_videos' files for one set: {prefix}_src_images/rgb_i.png, {prefix}_tgt_images/rgb_i.png, {prefix}_images/src_tgt_rgb_depth_i.png
    (src rgb | src depth | tgt rgb | tgt depth), and {prefix}_src_tgt_rgb_depth.mp4 when an ffmpeg executable is on PATH."""
    images_dir = os.path.join(output_dir, prefix + "_images")
    src_dir, tgt_dir = os.path.join(output_dir, prefix + "_src_images"), os.path.join(output_dir, prefix + "_tgt_images")
    for p in (images_dir, src_dir, tgt_dir):
        os.makedirs(p, exist_ok=True)
    for i in range(len(src_rgbs)):
        _png(os.path.join(src_dir, f"rgb_{i}.png"), src_rgbs[i])
        _png(os.path.join(tgt_dir, f"rgb_{i}.png"), tgt_rgbs[i])
        row = np.concatenate([src_rgbs[i], colorize_depth(src_depths[i].squeeze(-1)), tgt_rgbs[i], colorize_depth(tgt_depths[i].squeeze(-1))], axis=1)
        _png(os.path.join(images_dir, f"src_tgt_rgb_depth_{i}.png"), row)
    video = os.path.join(output_dir, prefix + "_src_tgt_rgb_depth.mp4")
    ffmpeg = shutil.which("ffmpeg")
    if ffmpeg is None:
        print(f"{prefix}: no ffmpeg on PATH, {os.path.basename(video)} skipped", flush=True)
        return
    subprocess.run([ffmpeg, "-y", "-loglevel", "error", "-framerate", "2", "-i", os.path.join(images_dir, "src_tgt_rgb_depth_%d.png"),
                    "-vcodec", "libx264", "-crf", "25", "-pix_fmt", "yuv420p", video], check=False)


def render_scene_views(output_dir: str, src_path: str, tgt_path: str, pose_gt: torch.Tensor, pose_pred: torch.Tensor, dataset: str, device,
                       renderer=None):
    """--render_views for one scene: the gt, aligned and unaligned sets of both blocks written under output_dir.  renderer(path, poses, K, W, H)
    -> (rgbs, depths) may be injected (tests); by default the blocks are loaded and rendered on `device`."""
    K, W, H = intrinsics(dataset)
    cams = {}
    if renderer is None:
        blocks = {p: load_render_block(p, device) for p in (src_path, tgt_path)}
        cams = {p: blocks[p][2]["camera_poses"] for p in blocks}

        def renderer(path, poses, K_, W_, H_):
            f, g, m = blocks[path]
            return render_views(f, g, m, poses, K_, W_, H_)
    else:
        cams = {p: block_camera_poses(p) for p in (src_path, tgt_path)}
    os.makedirs(output_dir, exist_ok=True)
    for prefix, (src_poses, tgt_poses) in pose_sets(cams[src_path], cams[tgt_path], pose_gt, pose_pred).items():
        src_rgbs, src_depths = renderer(src_path, src_poses, K, W, H)
        tgt_rgbs, tgt_depths = renderer(tgt_path, tgt_poses, K, W, H)
        write_render_set(output_dir, prefix, src_rgbs, src_depths, tgt_rgbs, tgt_depths)


def _stack_metrics(pred, gt):
    """Per-view PSNR / SSIM of two image stacks through the fused metrics kernel (one call): lists of floats."""
    from . import image_metrics as IM
    m = IM.image_metrics(torch.stack(list(pred)).contiguous(), torch.stack(list(gt)).contiguous())
    return m["psnr"].cpu().tolist(), m["ssim"].cpu().tolist()


def render_scene_merged(output_dir: str, src_path: str, tgt_path: str, pose_gt: torch.Tensor, pose_pred: torch.Tensor, dataset: str, device,
                        renderer=None, metrics=None):
    """--render_merged for one scene: both blocks rendered as ONE scene (render_pair_views) from every camera of both blocks, expressed in the
    target frame, under the ground-truth pose (prefix gt) and the predicted pose (prefix aligned): {prefix}_merged_images/rgb_i.png, depth_i.png
    and src_share_i.png (the source block's share of the opacity, grey).  merged_metrics.json holds PSNR / SSIM of the aligned views against
    the gt views — the photometric cost of the pose error; no ground-truth images are needed.
    renderer(pose, poses_c2w, K, W, H) -> (rgbs, depths, shares) and metrics(aligned_rgbs, gt_rgbs) -> (psnrs, ssims) may be injected (tests)."""
    import json
    K, W, H = intrinsics(dataset)
    if renderer is None:
        blocks = tuple(load_render_block(p, device) for p in (src_path, tgt_path))
        cams = [b[2]["camera_poses"] for b in blocks]

        def renderer(pose, poses, K_, W_, H_):
            return render_pair_views(blocks, pose, poses, K_, W_, H_)
    else:
        cams = [block_camera_poses(p) for p in (src_path, tgt_path)]
    metrics = metrics or _stack_metrics
    os.makedirs(output_dir, exist_ok=True)
    sets = pose_sets(cams[0], cams[1], pose_gt, pose_pred)
    stacks = {}
    for prefix, P in (("gt", pose_gt), ("aligned", pose_pred)):
        rgbs, depths, shares = renderer(P, sets[prefix][1], K, W, H)              # (P @ src cameras, tgt cameras): all in the target frame
        stacks[prefix] = rgbs
        d = os.path.join(output_dir, prefix + "_merged_images")
        os.makedirs(d, exist_ok=True)
        for i in range(len(rgbs)):
            rgb, depth, share = (np.asarray(v.cpu() if torch.is_tensor(v) else v) for v in (rgbs[i], depths[i], shares[i]))
            _png(os.path.join(d, f"rgb_{i}.png"), rgb)
            _png(os.path.join(d, f"depth_{i}.png"), colorize_depth(depth.squeeze(-1)))
            _png(os.path.join(d, f"src_share_{i}.png"), np.repeat(share.reshape(H, W, 1), 3, axis=2))
    psnr, ssim = metrics(stacks["aligned"], stacks["gt"])
    out = {"views": [{"psnr": float(p), "ssim": float(s)} for p, s in zip(psnr, ssim)],
           "psnr_mean": float(np.mean(psnr)), "ssim_mean": float(np.mean(ssim))}
    with open(os.path.join(output_dir, "merged_metrics.json"), "w") as f:
        json.dump(out, f, indent=2)
    return out


def block_camera_poses(path: str) -> torch.Tensor:
    """camera_poses [N,4,4] of a block checkpoint, read on the host without loading the field."""
    ngp.install_pickle_shims()
    try:
        snap = torch.load(path, map_location="cpu", weights_only=False, mmap=True)
    except (RuntimeError, ValueError):
        snap = torch.load(path, map_location="cpu", weights_only=False)
    return torch.as_tensor(snap["camera_poses"]).float().clone()
