"""A registered pair of NeRF blocks as ONE density field, and its surface mesh: the fused kernel of csrc/scene_field.hip in its K = 2 form
(dreg_pair_density; the lattice, the blend and the torch helpers are scene_field.py's) under the marching-cubes kernels of csrc/marching_cubes.hip.  The field is the scene the two-block renderer composites (render.render_pair_image): a block
contributes where its own occupancy cell is set, and where both do they share the point by the overlap weight.  Rule, kernel and measurements:
DESIGN.md §3i; CPU restatement: tests/pair_field_restatement.py."""
import math
from typing import Optional

import numpy as np
import torch

from . import lib as L
from . import mesh as M
from .scene_field import _lattice_dims, _pose34, blend_scene_attributes, grid_covered, points_to_frame, scene_lattice


def pair_lattice(src_aabb, tgt_aabb, pose, resolution: int):
    """(origin, spacing, (nx, ny, nz)) of the lattice a pair is meshed on, in the TARGET frame: scene_lattice over the target model aabb and the
    source model aabb moved by the pose."""
    return scene_lattice([src_aabb, tgt_aabb], [pose, None], resolution)


def blend_vertex_attributes(w_src, w_tgt, sigma_src, sigma_tgt, R, grad_src, grad_tgt, color_src=None, color_tgt=None):
    """Per-vertex attributes of a pair mesh from the two blocks' own, all [V] / [V,3] tensors of one dtype: blend_scene_attributes with K = 2 and
    the source block's rotation R.  With a_b = w_b sigma_b, g = w_S R grad_S + w_T grad_T (grad_S in the source frame), normal = -g / |g|; colour
    = (a_S c_S + a_T c_T) / (a_S + a_T) (one block's own colour, bit for bit, where the other's a is 0) and weight_src = a_S / (a_S + a_T), zeros
    where a denominator is 0.  Returns (normals, colors or None, weight_src)."""
    colors = None if color_src is None or color_tgt is None else [color_src, color_tgt]
    normals, colors, share = blend_scene_attributes(torch.stack([w_src, w_tgt], dim=1), torch.stack([sigma_src, sigma_tgt], dim=1), [R, None],
                                                    [grad_src, grad_tgt], colors)
    return normals, colors, share[:, 0]


class PairField:
    """The density field of a registered pair: PairField(src_field, src_grid, tgt_field, tgt_grid, pose, src_center, tgt_center, power=4.0).
    Grids are render.BlockGrid or ngp.OccupancyGrid (as render_pair_image takes them); pose = [R|t] ([3,4] or [4,4]) maps the source frame to the
    target frame, in which the field lives; *_center: the centroid of the block's cameras in its own frame.  The fp64 pose is rounded to fp32 once
    (self.R, self.t: what the kernel receives)."""

    def __init__(self, src_field, src_grid, tgt_field, tgt_grid, pose, src_center, tgt_center, power: float = 4.0):
        from . import render
        for f in (src_field, tgt_field):
            if getattr(f, "unbounded", False):
                raise NotImplementedError("PairField: the contracted (unbounded) field is not implemented")
        for g in (src_grid, tgt_grid):
            if getattr(getattr(g, "contraction_type", None), "name", "AABB") != "AABB":
                raise NotImplementedError("PairField: only ContractionType.AABB occupancy grids are supported (DESIGN.md: no contraction)")
        dev = tgt_field.aabb.device
        if dev.type != "cuda" or src_field.aabb.device != dev:
            raise ValueError("PairField: both blocks must be on the same GPU (there is no CPU path)")
        if not (math.isfinite(float(power)) and float(power) > 0.0):
            raise ValueError(f"PairField: power {power} must be finite and positive")
        self.src, self.tgt, self.device, self.power = src_field, tgt_field, dev, float(power)
        self.pose = _pose34(pose)
        self.R = self.pose[:, :3].astype(np.float32)
        self.t = self.pose[:, 3].astype(np.float32)
        self._pose12 = (L.c_float * 12)(*[float(v) for v in self.R.reshape(-1)], *[float(v) for v in self.t])
        self.centers = [[float(v) for v in torch.as_tensor(c).reshape(-1).tolist()] for c in (src_center, tgt_center)]
        self._grids = [render._grid_parts(g, dev)[:2] for g in (src_grid, tgt_grid)]        # (roi as 6 host floats, uint8 occupancy on the device)

    def _block_args(self, k: int, keep: list):
        field = (self.src, self.tgt)[k]
        roi, b8 = self._grids[k]
        arrs = [L.f6(roi), L.f6(field._aabb_host()), L.f3(self.centers[k])]
        keep.extend([b8, field._prepared()] + arrs)
        return [L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], *field.density_ptrs(), *field._levels, *arrs]

    def _run(self, x, n, origin, spacing, dims, parts):
        lib = L.load()
        with torch.cuda.device(self.device):
            outs = [torch.empty(n, dtype=torch.float32, device=self.device) for _ in range(5 if parts else 1)]
            keep = []
            src_args, tgt_args = self._block_args(0, keep), self._block_args(1, keep)
            org = None if origin is None else L.f3(origin)
            spc = None if spacing is None else L.f3(spacing)
            L.check(lib.dreg_pair_density(L.ptr(x) if x is not None and n else None, n if x is not None else 0, org, spc, *dims, *src_args, *tgt_args,
                                          self._pose12, self.power, *[L.ptr(o) if n else None for o in outs], *([None] * (5 - len(outs))), L.stream()),
                    "dreg_pair_density")
        return outs

    @torch.no_grad()
    def query(self, x: torch.Tensor, parts: bool = False):
        """x [...,3] in the target frame -> sigma [...]; with parts=True (sigma, w_src, w_tgt, sigma_src, sigma_tgt): the blocks' weights (0, 1, or
        w and 1 - w where both cover the point) and m_b ? sigma_b : 0."""
        if not x.is_cuda:
            raise ValueError("PairField.query: x must be on the GPU (there is no CPU path)")
        shp = x.shape[:-1]
        x = x.reshape(-1, 3).to(self.device).float().contiguous()
        outs = [o.view(*shp) for o in self._run(x, x.shape[0], None, None, (0, 0, 0), parts)]
        return tuple(outs) if parts else outs[0]

    @torch.no_grad()
    def sample_lattice(self, origin, spacing, dims) -> torch.Tensor:
        """The pair density at the nodes origin + (float)i * spacing of an nx x ny x nz lattice: fp32 [nz,ny,nx].  No position tensor is formed."""
        nx, ny, nz = _lattice_dims(dims)
        return self._run(None, nx * ny * nz, origin, spacing, (nx, ny, nz), False)[0].view(nz, ny, nx)

    def lattice(self, resolution: int):
        return pair_lattice(self.src._aabb_host(), self.tgt._aabb_host(), self.pose, resolution)

    def covered(self, k: int, x: torch.Tensor) -> torch.Tensor:
        """Own coverage m_b of block k (0 = source, 1 = target) at x [N,3] fp32 of THAT block's frame (scene_field.grid_covered)."""
        return grid_covered(*self._grids[k], x)

    def points_to_source(self, x: torch.Tensor) -> torch.Tensor:
        """x [N,3] fp32 of the target frame in the source frame (scene_field.points_to_frame: the kernel's bits)."""
        return points_to_frame(self.R, self.t, x)


@torch.no_grad()
def pair_mesh(pf: PairField, resolution: int = 256, level: Optional[float] = None, normals: bool = True, colors: bool = True) -> dict:
    """Surface mesh of a registered pair in the target frame: the pair density on pair_lattice(resolution) (one fused launch), marching cubes at `level`
    (default mesh.DENSITY_THRE), then per vertex — from the existing kernels, at the V vertices only — the blended field normal, the blended mean
    colour over the extraction's 18 fixed directions (each block's in its own frame, as merged_scene_mesh reuses colours) and weight_src, the
    source block's share of the density (blend_vertex_attributes).  Returns block_mesh's dict plus "weight_src" fp32 [V] and "dims"."""
    from . import ngp
    level = M.DENSITY_THRE if level is None else float(level)
    origin, spacing, dims = pf.lattice(resolution)
    values = pf.sample_lattice(origin, spacing, dims)
    verts, faces = M.marching_cubes(values, level, origin, spacing)
    out = {"verts": verts, "faces": faces, "normals": None, "colors": None, "weight_src": None, "level": level, "origin": origin, "spacing": spacing,
           "resolution": resolution, "dims": dims}
    V = verts.shape[0]
    if V == 0:
        out["weight_src"] = verts.new_zeros(0)
        out["normals"] = verts.new_zeros(0, 3) if normals else None
        out["colors"] = verts.new_zeros(0, 3) if colors else None
        return out
    _, w_s, w_t, s_s, s_t = pf.query(verts, parts=True)
    xs = pf.points_to_source(verts).contiguous()
    if normals:
        g_s, g_t = pf.src.query_density_grad(xs)[1], pf.tgt.query_density_grad(verts)[1]
    else:
        g_s = g_t = torch.zeros_like(verts)
    c_s = c_t = None
    if colors:
        dirs = ngp.SampleGrid._generate_fixed_viewing_directions().to(verts.device).float().contiguous()
        c_s = pf.src.query_rgb_mean(pf.src.query_raw(xs)[1], dirs)
        c_t = pf.tgt.query_rgb_mean(pf.tgt.query_raw(verts)[1], dirs)
    nrm, col, wsrc = blend_vertex_attributes(w_s, w_t, s_s, s_t, torch.from_numpy(pf.R), g_s, g_t, c_s, c_t)
    out["weight_src"] = wsrc
    out["normals"] = nrm if normals else None
    out["colors"] = col
    return out


def merged_field_scene_mesh(output_dir: str, src_path: str, tgt_path: str, pose_gt: torch.Tensor, pose_pred: torch.Tensor, dev, resolution: int = 256,
                            level: Optional[float] = None, power: float = 4.0) -> dict:
    """eval_nerf_regtr.py --merged_mesh_field for one scene: ONE closed surface of the pair per pose — merged_field_mesh_pred.ply under the
    predicted pose, merged_field_mesh_gt.ply under the known one — and merged_field_mesh.json with V, F, area and volume of both.  Poses are
    source -> target, the camera centroids come from the checkpoints' camera_poses, as --render_merged takes them."""
    import json
    import os
    from . import vis_dump
    from .render import load_render_block
    (sf, sg, sm), (tf, tg, tm) = (load_render_block(p, dev) for p in (src_path, tgt_path))
    centers = [torch.as_tensor(m["camera_poses"]).float()[:, :3, 3].mean(0).cpu() for m in (sm, tm)]
    os.makedirs(output_dir, exist_ok=True)
    out, stats = {}, {}
    cpu = lambda t: None if t is None else t.detach().cpu().numpy()
    for name, P in (("pred", pose_pred), ("gt", pose_gt)):
        m = pair_mesh(PairField(sf, sg, tf, tg, P, centers[0], centers[1], power=power), resolution, level)
        vis_dump.write_mesh_ply(os.path.join(output_dir, f"merged_field_mesh_{name}.ply"), cpu(m["verts"]), cpu(m["faces"]), cpu(m["colors"]), cpu(m["normals"]))
        area, vol = M.mesh_area_volume(m["verts"], m["faces"])
        stats[name] = {"V": int(m["verts"].shape[0]), "F": int(m["faces"].shape[0]), "area": area, "volume": vol}
        out[name] = m
    stats.update(level=out["gt"]["level"], resolution=int(resolution), power=float(power))
    with open(os.path.join(output_dir, "merged_field_mesh.json"), "w") as f:
        json.dump(stats, f, indent=2)
    out["stats"] = stats
    return out
