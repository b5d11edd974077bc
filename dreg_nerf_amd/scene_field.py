"""A registered SCENE of K NeRF blocks (1 <= K <= 4) as ONE density field, and its surface mesh: the fused kernel of csrc/scene_field.hip under the
marching-cubes kernels of csrc/marching_cubes.hip.  The field is the scene the K-block renderer composites (render.render_scene_image, DESIGN.md
§3j): a block contributes where its own occupancy cell is set, and where several do they share the point by the overlap weight.  The
pair's field (pair_field.py) is the K = 2 form and takes its lattice, blend and helpers from here; rule, kernel and measurements: DESIGN.md §3k;
CPU restatement: tests/scene_field_restatement.py."""
import ctypes
import math
from typing import Optional

import numpy as np
import torch

from . import lib as L
from . import mesh as M

MAX_DIM, MAX_NODES = 1024, 1 << 28      # the density entries' and dreg_mc_count's lattice limits


def _pose34(pose) -> np.ndarray:
    """A [3,4] or [4,4] pose as fp64 [3,4] on the host."""
    P = (pose.detach().double().cpu().numpy() if torch.is_tensor(pose) else np.asarray(pose, dtype=np.float64)).reshape(-1, 4)
    if P.shape[0] not in (3, 4):
        raise ValueError(f"pose must be [3,4] or [4,4], got {tuple(P.shape)}")
    return P[:3].copy()


def _f32_up(v: float) -> float:
    f = np.float32(v)
    return float(f if float(f) >= v else np.nextafter(f, np.float32(np.inf)))


def _f32_down(v: float) -> float:
    f = np.float32(v)
    return float(f if float(f) <= v else np.nextafter(f, np.float32(-np.inf)))


def _lattice_dims(dims):
    """(nx, ny, nz) as ints, refused as the density entries refuse them."""
    nx, ny, nz = (int(v) for v in dims)
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) > MAX_DIM or nx * ny * nz > MAX_NODES:
        raise ValueError(f"sample_lattice: lattice {nx} x {ny} x {nz}: every dimension must be in [2, 1024] and the nodes at most 2^28")
    return nx, ny, nz


def grid_covered(roi, b8: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Own coverage of a block with occupancy b8 (uint8 [rx,ry,rz]) over roi (6 host floats) at x [N,3] fp32 of THAT block's frame, in torch fp32
    elementwise ops: inside the roi (0 <= u <= 1 on all axes) and the cell clamp(floor(u res), 0, res - 1) set.  Not the hot path (tools,
    composition baseline)."""
    lo = x.new_tensor(roi[:3])
    u = (x - lo) / (x.new_tensor(roi[3:]) - lo)
    inside = ((u >= 0) & (u <= 1)).all(dim=1)
    res = x.new_tensor([float(v) for v in b8.shape])
    ci = torch.minimum(torch.floor(torch.where(inside[:, None], u, torch.zeros_like(u)) * res).clamp(min=0), res - 1).long()
    return inside & (b8[ci[:, 0], ci[:, 1], ci[:, 2]] != 0)


def points_to_frame(Rf, tf, x: torch.Tensor) -> torch.Tensor:
    """x [N,3] fp32 of the scene frame in the frame of a block with the fp32 pose [Rf|tf] (block -> scene), by the kernel's own expression in
    torch fp32 elementwise ops (the same bits)."""
    d = [x[:, k] - float(tf[k]) for k in range(3)]
    return torch.stack([(float(Rf[0, k]) * d[0] + float(Rf[1, k]) * d[1]) + float(Rf[2, k]) * d[2] for k in range(3)], dim=1)


def _scene_box64(aabbs, poses, who: str):
    """(lo, hi) fp64 of the box of all K model aabbs, each moved (its eight corners) by its pose (block -> scene; None: the aabb as given)."""
    aabbs, poses = list(aabbs), list(poses)
    if len(aabbs) != len(poses) or not 1 <= len(aabbs) <= L.SCENE_MAX_BLOCKS:
        raise ValueError(f"{who}: {len(aabbs)} aabbs and {len(poses)} poses (1 to {L.SCENE_MAX_BLOCKS} blocks, one pose or None per block)")
    los, his = [], []
    for aabb, pose in zip(aabbs, poses):
        s = np.asarray([float(v) for v in (aabb.tolist() if torch.is_tensor(aabb) else aabb)], dtype=np.float64)
        if pose is None:
            los.append(s[:3])
            his.append(s[3:])
            continue
        P = _pose34(pose)
        corners = np.array([[s[3 * i], s[3 * j + 1], s[3 * k + 2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
        moved = corners @ P[:, :3].T + P[:, 3]
        los.append(moved.min(axis=0))
        his.append(moved.max(axis=0))
    return np.min(np.stack(los), axis=0), np.max(np.stack(his), axis=0)


def scene_box(aabbs, poses):
    """The box of a registered scene in the SCENE frame, as 6 fp32-exact Python floats (lo | hi): in fp64 the box of all K model aabbs, each moved
    (its eight corners) by its pose (block -> scene; None: the aabb as given) — the box scene_lattice spans its lattice over —, rounded OUTWARD
    to fp32 (lo down, hi up).  It is not made cubic.  ValueError when it spans no volume on some axis."""
    lo, hi = _scene_box64(aabbs, poses, "scene_box")
    ext = hi - lo
    if not (np.isfinite(ext).all() and ext.min() > 0):
        raise ValueError("scene_box: the aabbs span no volume")
    return [_f32_down(float(v)) for v in lo] + [_f32_up(float(v)) for v in hi]


def scene_lattice(aabbs, poses, resolution: int):
    """(origin, spacing, (nx, ny, nz)) of the lattice a scene is meshed on, in the SCENE frame.  In fp64: the box of all K model aabbs, each moved
    (its eight corners) by its pose (block -> scene; None: the aabb as given); h = the box's longest extent / resolution (cubic cells); origin =
    lo - h and n_k = ceil(ext_k / h) + 3 nodes (resolution + 3 on the longest axis), so the first and the last node of every axis lie at least h
    outside every aabb: the lattice's shell is exactly 0 and every level > 0 gives a closed mesh.  origin and spacing are fp32-exact Python floats;
    the rounding is directed (h up, after one part in 2^20 is added to it; origin down from lo - h) so that it cannot eat the margin.  ValueError
    when a dimension exceeds 1024 or the nodes exceed 2^28."""
    if int(resolution) < 1:
        raise ValueError(f"scene_lattice: resolution {resolution} must be >= 1")
    resolution = int(resolution)
    lo, hi = _scene_box64(aabbs, poses, "scene_lattice")
    ext = hi - lo
    if not (np.isfinite(ext).all() and ext.max() > 0):
        raise ValueError("scene_lattice: the aabbs span no volume")
    h = float(ext.max()) / resolution
    longest = int(np.argmax(ext))
    dims = tuple(resolution + 3 if k == longest else int(math.ceil(ext[k] / h)) + 3 for k in range(3))
    if max(dims) > MAX_DIM:
        raise ValueError(f"scene_lattice: {dims[0]} x {dims[1]} x {dims[2]} nodes: a dimension exceeds {MAX_DIM}")
    if dims[0] * dims[1] * dims[2] > MAX_NODES:
        raise ValueError(f"scene_lattice: {dims[0]} x {dims[1]} x {dims[2]} nodes exceed 2^28")
    h32 = _f32_up(h * (1.0 + 2.0 ** -20))
    origin = [_f32_down(float(lo[k]) - h32) for k in range(3)]
    return origin, [h32, h32, h32], dims


def blend_scene_attributes(weight_block, sigma_block, Rs, grads, colors=None):
    """Per-vertex attributes of a scene mesh from the K blocks' own: weight_block / sigma_block [V,K] (SceneField.query's parts), Rs a list of K
    rotations ([3,3], block -> scene) or None (the block's frame is the scene's), grads a list of K [V,3] density gradients each in its block's
    frame, colors a list of K [V,3] or None.  With a_b = omega_b sigma_b: g = sum_b omega_b R_b grad_b (the gradient of the overlap weight is
    ignored), normal = -g / |g| (zeros where g vanishes or is not finite); colour = sum_b a_b c_b / sum_b a_b (one block's own colour, bit for bit,
    where it alone has a_b != 0) and share [V,K] = a_b / sum a, both zeros where the denominator is 0.  All sums run in block order.  Returns
    (normals, colors or None, share); pair_field.blend_vertex_attributes is the call with K = 2 and Rs = [R, None] (share[:,0] = weight_src)."""
    K = weight_block.shape[1]
    g = None
    for b in range(K):
        gb = grads[b]
        if Rs[b] is not None:
            R = torch.as_tensor(Rs[b], dtype=gb.dtype, device=gb.device)
            gb = torch.stack([R[k, 0] * gb[:, 0] + R[k, 1] * gb[:, 1] + R[k, 2] * gb[:, 2] for k in range(3)], dim=1)   # elementwise: no GEMM library in the path
        term = weight_block[:, b, None] * gb
        g = term if g is None else g + term
    norm = g.norm(dim=1, keepdim=True)
    ok = (norm > 0) & torch.isfinite(norm)
    normals = torch.where(ok, -g / torch.where(ok, norm, torch.ones_like(norm)), torch.zeros_like(g))
    a = [weight_block[:, b] * sigma_block[:, b] for b in range(K)]
    den = a[0]
    for b in range(1, K):
        den = den + a[b]
    has = den > 0
    safe = torch.where(has, den, torch.ones_like(den))
    share = torch.stack([torch.where(has, a[b] / safe, torch.zeros_like(den)) for b in range(K)], dim=1)
    out = None
    if colors is not None:
        num = a[0][:, None] * colors[0]
        for b in range(1, K):
            num = num + a[b][:, None] * colors[b]
        mix = num / safe[:, None]
        # where one block alone carries the density the colour is that block's own, bit for bit ((a c) / a may differ from c by a rounding)
        carriers = sum((a[b] != 0).to(torch.int32) for b in range(K))
        for b in range(K):
            mix = torch.where(((a[b] != 0) & (carriers == 1))[:, None], colors[b], mix)
        out = torch.where(has[:, None], mix, torch.zeros_like(colors[0]))
    return normals, out, share


class SceneField:
    """The density field of a registered scene: SceneField(blocks, power=4.0) with blocks a list of 1 to 4 (field, grid, center, pose_or_None).
    Grids are render.BlockGrid or ngp.OccupancyGrid; center: the centroid of the block's cameras in its own frame; pose = G_b = [R|t] ([3,4] or
    [4,4]) maps the block's frame to the scene frame, in which the field lives, or None: the block's frame IS the scene's and points reach it
    untouched.  Each fp64 pose is rounded to fp32 once (self.R[b], self.t[b]: what the kernel receives; None without a pose).  metas (optional,
    one dict per block with 'camera_poses' [N,4,4] and 'render_step_size', optionally 'aabb' and 'alpha_thre': a checkpoint's meta data) is what
    extract_grid(surface=True) marches the blocks' own cameras with."""

    def __init__(self, blocks, power: float = 4.0, metas=None):
        from . import render
        blocks = list(blocks)
        if not 1 <= len(blocks) <= L.SCENE_MAX_BLOCKS:
            raise ValueError(f"SceneField: {len(blocks)} blocks (1 to {L.SCENE_MAX_BLOCKS} make one field)")
        for f, g, _, _ in blocks:
            if getattr(f, "unbounded", False):
                raise NotImplementedError("SceneField: the contracted (unbounded) field is not implemented")
            if getattr(getattr(g, "contraction_type", None), "name", "AABB") != "AABB":
                raise NotImplementedError("SceneField: only ContractionType.AABB occupancy grids are supported (DESIGN.md: no contraction)")
        dev = blocks[0][0].aabb.device
        if dev.type != "cuda" or any(b[0].aabb.device != dev for b in blocks[1:]):
            raise ValueError("SceneField: all blocks must be on the same GPU (there is no CPU path)")
        if not (math.isfinite(float(power)) and float(power) > 0.0):
            raise ValueError(f"SceneField: power {power} must be finite and positive")
        self.K, self.device, self.power = len(blocks), dev, float(power)
        self.fields = [b[0] for b in blocks]
        self.poses = [None if b[3] is None else _pose34(b[3]) for b in blocks]
        self.R = [None if P is None else P[:, :3].astype(np.float32) for P in self.poses]
        self.t = [None if P is None else P[:, 3].astype(np.float32) for P in self.poses]
        self._pose12 = [None if P is None else (L.c_float * 12)(*[float(v) for v in R.reshape(-1)], *[float(v) for v in t])
                        for P, R, t in zip(self.poses, self.R, self.t)]
        self.centers = [[float(v) for v in torch.as_tensor(b[2]).reshape(-1).tolist()] for b in blocks]
        self._grids = [render._grid_parts(b[1], dev)[:2] for b in blocks]        # (roi as 6 host floats, uint8 occupancy on the device)
        if metas is not None and len(metas) != len(blocks):
            raise ValueError(f"SceneField: {len(metas)} metas for {len(blocks)} blocks")
        self.metas = None if metas is None else list(metas)
        self._dirbias = None                                                     # per block, made by the first extract_grid

    def _block_array(self, keep: list):
        arr = (L.FieldBlock * self.K)()
        names = [n for n, _ in L.FieldBlock._fields_]
        for k, field in enumerate(self.fields):
            roi, b8 = self._grids[k]
            arrs = [L.f6(roi), L.f6(field._aabb_host()), L.f3(self.centers[k])]
            keep.extend([b8, field._prepared()] + arrs)
            args = [L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], *field.density_ptrs(), *field._levels, *arrs, self._pose12[k]]
            for name, v in zip(names, args):
                setattr(arr[k], name, ctypes.cast(v, ctypes.c_void_p) if isinstance(v, ctypes.Array) else v)
        return arr

    def _radiance_array(self, keep: list):
        """The HOST array of dreg_radiance_block for dreg_scene_voxel_grid: every block's dreg_field_block, its colour net and the dir-bias buffer of
        SampleGrid's 18 fixed viewing directions (made once per field: the weights of a SceneField's blocks are taken as frozen)."""
        from . import ngp
        if self._dirbias is None:
            dirs = ngp.SampleGrid._generate_fixed_viewing_directions().to(self.device).float().contiguous()
            self._dirbias = [f.dir_bias(dirs) for f in self.fields]             # views of the [2 * 18, 64] buffers dreg_ngp_dir_bias wrote
        fb = self._block_array(keep)
        arr = (L.RadianceBlock * self.K)()
        for k, field in enumerate(self.fields):
            ctypes.memmove(ctypes.addressof(arr[k].field), ctypes.addressof(fb[k]), ctypes.sizeof(L.FieldBlock))
            arr[k].cw1, arr[k].cw2, arr[k].cw3 = field.color_ptrs()
            arr[k].dirbias = self._dirbias[k].data_ptr()
        keep.append(self._dirbias)
        return arr

    @torch.no_grad()
    def extract_grid(self, resolution=128, aabb=None, jitter=None, density_thre: float = 0.7, delta: float = 1e-2, surface: bool = False,
                     cut_off: float = 0.5) -> dict:
        """The registered scene as ONE voxel grid in the format of a block's voxel_grid.pt / voxel_mask.pt (csrc/scene_grid.hip, one fused launch;
        rule: DESIGN.md §3l).  resolution: an int or (rx, ry, rz); aabb: the grid's box in the scene frame (6 floats; default scene_box of the
        blocks); jitter: [rx ry rz, 3] (or [rx,ry,rz,3]) fp32 offsets of the samples within their cells, None = the cell centres.  Returns
        {"voxel_grid" fp32 [rx,ry,rz,7] = (xyz | rgb | alpha) at kept cells and 0 elsewhere, "keep" bool [rx,ry,rz] (sigma > density_thre),
        "sigma" fp32 [rx,ry,rz], "voxel_mask" int64 ascending flat indices of the kept cells, "aabb"}.  surface=True (needs metas): a kept cell
        stays iff, for some block b that covers it, visibility.surface_visibility of the cell's x_b from b's own cameras through b's own field
        says visible; rows of cells that fail are zeroed and leave the mask.  Occlusion of one block's cameras by another block is ignored."""
        res = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
        if len(res) != 3 or min(res) < 1 or max(res) > MAX_DIM or res[0] * res[1] * res[2] > MAX_NODES:
            raise ValueError(f"extract_grid: resolution {resolution}: three dimensions in [1, 1024] and at most 2^28 cells")
        box = self.box() if aabb is None else [float(np.float32(v)) for v in (aabb.tolist() if torch.is_tensor(aabb) else aabb)]
        if len(box) != 6 or not all(math.isfinite(v) for v in box) or not all(np.float32(box[3 + k]) - np.float32(box[k]) > 0 for k in range(3)):
            raise ValueError(f"extract_grid: aabb {box} must be 6 finite floats with a positive extent on every axis")
        if not (math.isfinite(float(density_thre)) and math.isfinite(float(delta)) and float(delta) > 0.0):
            raise ValueError(f"extract_grid: density_thre {density_thre} must be finite and delta {delta} finite and positive")
        if surface and self.metas is None:
            raise ValueError("extract_grid: surface=True needs the blocks' metas (camera_poses, render_step_size)")
        n = res[0] * res[1] * res[2]
        if jitter is not None:
            if not jitter.is_cuda or jitter.numel() != 3 * n:
                raise ValueError(f"extract_grid: jitter must be on the GPU with {n} x 3 entries")
            jitter = jitter.reshape(n, 3).to(self.device).float().contiguous()
        lib = L.load()
        with torch.cuda.device(self.device):
            grid = torch.empty(n, 7, dtype=torch.float32, device=self.device)
            keep8 = torch.empty(n, dtype=torch.uint8, device=self.device)
            sigma = torch.empty(n, dtype=torch.float32, device=self.device)
            alive = []
            arr = self._radiance_array(alive)
            L.check(lib.dreg_scene_voxel_grid(res[0], res[1], res[2], L.f6(box), L.ptr(jitter), self.K, ctypes.cast(arr, ctypes.c_void_p), self.power,
                                              float(delta), float(density_thre), L.ptr(grid), L.ptr(keep8), L.ptr(sigma), L.stream()), "dreg_scene_voxel_grid")
            keep = keep8.view(torch.bool)
            if surface:
                keep = self._surface_keep(grid, keep, cut_off)
        return {"voxel_grid": grid.view(*res, 7), "keep": keep.view(*res), "sigma": sigma.view(*res), "voxel_mask": torch.nonzero(keep)[:, 0], "aabb": box}

    def _surface_keep(self, grid, keep, cut_off):
        """extract_grid's surface mask, a composition of the existing marcher: per block b, the kept cells b covers are marched from b's own cameras
        through b's own field; cells no block sees are zeroed in `grid` (in place).  Returns the new keep [n]."""
        from . import visibility
        idx = torch.nonzero(keep)[:, 0]
        w = grid[idx, :3].contiguous()
        seen = torch.zeros(idx.shape[0], dtype=torch.bool, device=self.device)
        for b, (field, meta) in enumerate(zip(self.fields, self.metas)):
            xb = self.points_to_block(b, w).contiguous()
            sel = torch.nonzero(self.covered(b, xb))[:, 0]
            if sel.numel() == 0:
                continue
            roi, b8 = self._grids[b]
            cams = torch.as_tensor(meta["camera_poses"])[..., :3, 3].to(self.device)
            vis = visibility.surface_visibility(xb[sel].contiguous(), cams, field, b8, roi, meta.get("aabb", roi), meta["render_step_size"], cut_off, 1e-4,
                                                float(meta.get("alpha_thre") or 0.0))
            seen[sel] |= vis.view(-1).bool()
        grid[idx[~seen]] = 0.0
        out = keep.clone()
        out[idx[~seen]] = False
        return out

    def box(self):
        return scene_box([f._aabb_host() for f in self.fields], self.poses)

    def _run(self, x, n, origin, spacing, dims, parts):
        lib = L.load()
        with torch.cuda.device(self.device):
            sigma = torch.empty(n, dtype=torch.float32, device=self.device)
            wb, sb = ((torch.empty(n, self.K, dtype=torch.float32, device=self.device) for _ in range(2)) if parts else (None, None))
            keep = []
            arr = self._block_array(keep)
            org = None if origin is None else L.f3(origin)
            spc = None if spacing is None else L.f3(spacing)
            L.check(lib.dreg_scene_density(L.ptr(x) if x is not None and n else None, n if x is not None else 0, org, spc, *dims, self.K,
                                           ctypes.cast(arr, ctypes.c_void_p), self.power, L.ptr(sigma) if n else None,
                                           L.ptr(wb) if parts and n else None, L.ptr(sb) if parts and n else None, L.stream()), "dreg_scene_density")
        return sigma, wb, sb

    @torch.no_grad()
    def query(self, x: torch.Tensor, parts: bool = False):
        """x [...,3] in the scene frame -> sigma [...]; with parts=True (sigma, weight_block [...,K], sigma_block [...,K]): the blocks' weights (0
        where a block does not cover the point, 1 where it alone does, shares that sum to 1 where several do) and m_b ? sigma_b : 0."""
        if not x.is_cuda:
            raise ValueError("SceneField.query: x must be on the GPU (there is no CPU path)")
        shp = x.shape[:-1]
        x = x.reshape(-1, 3).to(self.device).float().contiguous()
        sigma, wb, sb = self._run(x, x.shape[0], None, None, (0, 0, 0), parts)
        return (sigma.view(*shp), wb.view(*shp, self.K), sb.view(*shp, self.K)) if parts else sigma.view(*shp)

    @torch.no_grad()
    def sample_lattice(self, origin, spacing, dims) -> torch.Tensor:
        """The scene density at the nodes origin + (float)i * spacing of an nx x ny x nz lattice: fp32 [nz,ny,nx].  No position tensor is formed."""
        nx, ny, nz = _lattice_dims(dims)
        return self._run(None, nx * ny * nz, origin, spacing, (nx, ny, nz), False)[0].view(nz, ny, nx)

    def lattice(self, resolution: int):
        return scene_lattice([f._aabb_host() for f in self.fields], self.poses, resolution)

    def covered(self, b: int, x_b: torch.Tensor) -> torch.Tensor:
        """Own coverage m_b of block b at x_b [N,3] fp32 of THAT block's frame (grid_covered)."""
        return grid_covered(*self._grids[b], x_b)

    def points_to_block(self, b: int, x: torch.Tensor) -> torch.Tensor:
        """x [N,3] fp32 of the scene frame in block b's frame (points_to_frame: the kernel's bits); x itself where the block has no pose."""
        return x if self.poses[b] is None else points_to_frame(self.R[b], self.t[b], x)


@torch.no_grad()
def scene_mesh(sf: SceneField, resolution: int = 256, level: Optional[float] = None, normals: bool = True, colors: bool = True) -> dict:
    """Surface mesh of a registered scene in the scene frame (pair_field.pair_mesh for K blocks): the scene density on scene_lattice(resolution)
    (one fused launch), marching cubes at `level` (default mesh.DENSITY_THRE), then per vertex — from the existing kernels, at the V vertices only
    — the blended field normal, the blended mean colour over the extraction's 18 fixed directions (each block's in its own frame) and share
    [V,K], the blocks' shares of the density (blend_scene_attributes).  Returns pair_mesh's dict with "share" in place of "weight_src"."""
    from . import ngp
    level = M.DENSITY_THRE if level is None else float(level)
    origin, spacing, dims = sf.lattice(resolution)
    values = sf.sample_lattice(origin, spacing, dims)
    verts, faces = M.marching_cubes(values, level, origin, spacing)
    out = {"verts": verts, "faces": faces, "normals": None, "colors": None, "share": None, "level": level, "origin": origin, "spacing": spacing,
           "resolution": resolution, "dims": dims}
    V = verts.shape[0]
    if V == 0:
        out["share"] = verts.new_zeros(0, sf.K)
        out["normals"] = verts.new_zeros(0, 3) if normals else None
        out["colors"] = verts.new_zeros(0, 3) if colors else None
        return out
    _, wb, sb = sf.query(verts, parts=True)
    xb = [sf.points_to_block(b, verts).contiguous() for b in range(sf.K)]
    if normals:
        grads = [f.query_density_grad(x)[1] for f, x in zip(sf.fields, xb)]
    else:
        grads = [torch.zeros_like(verts) for _ in range(sf.K)]
    cols = None
    if colors:
        dirs = ngp.SampleGrid._generate_fixed_viewing_directions().to(verts.device).float().contiguous()
        cols = [f.query_rgb_mean(f.query_raw(x)[1], dirs) for f, x in zip(sf.fields, xb)]
    nrm, col, share = blend_scene_attributes(wb, sb, [None if R is None else torch.from_numpy(R) for R in sf.R], grads, cols)
    out["share"] = share
    out["normals"] = nrm if normals else None
    out["colors"] = col
    return out


def registered_scene_mesh(output_dir: str, scene, G_gt, G_sync, dataset: str, device, resolution: int = 256, level: Optional[float] = None,
                          power: float = 4.0) -> dict:
    """eval_nerf_regtr.py --scene_mesh_field for one scene: ONE closed surface of ALL its blocks per pose set, in the anchor's frame —
    scene_field_mesh_gt.ply under the ground-truth G and scene_field_mesh_aligned.ply under the synchronised G — and scene_field_mesh.json with K
    and, for both, V, F, area and volume.  The blocks are loaded, the camera centroids taken from the checkpoints' camera_poses and every block
    (the anchor too) given its G_b, as scene_reg.render_registered_scene does; `dataset` is accepted for the same signature."""
    import json
    import os
    from . import vis_dump
    from .render import load_render_block
    loaded = [load_render_block(b["nerf_path"], device) for b in scene]
    centers = [torch.as_tensor(m["camera_poses"]).float()[:, :3, 3].mean(0).cpu() for _, _, m in loaded]
    G_gt, G_sync = torch.as_tensor(G_gt).double().cpu(), torch.as_tensor(G_sync).double().cpu()
    os.makedirs(output_dir, exist_ok=True)
    out, stats = {}, {"K": len(loaded)}
    cpu = lambda t: None if t is None else t.detach().cpu().numpy()
    for name, G in (("gt", G_gt), ("aligned", G_sync)):
        sf = SceneField([(f, g, centers[b], G[b]) for b, (f, g, _) in enumerate(loaded)], power=power)
        m = scene_mesh(sf, resolution, level)
        vis_dump.write_mesh_ply(os.path.join(output_dir, f"scene_field_mesh_{name}.ply"), cpu(m["verts"]), cpu(m["faces"]), cpu(m["colors"]), cpu(m["normals"]))
        area, vol = M.mesh_area_volume(m["verts"], m["faces"])
        stats[name] = {"V": int(m["verts"].shape[0]), "F": int(m["faces"].shape[0]), "area": area, "volume": vol}
        out[name] = m
    stats.update(level=out["gt"]["level"], resolution=int(resolution), power=float(power))
    with open(os.path.join(output_dir, "scene_field_mesh.json"), "w") as f:
        json.dump(stats, f, indent=2)
    out["stats"] = stats
    return out
