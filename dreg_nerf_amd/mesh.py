"""Surface meshes of NeRF blocks: the fused marching-cubes kernels of csrc/marching_cubes.hip on the block's own density field.  The reference's
mesh export (convert_sdf_samples_to_ply, utils.py:284-344) calls skimage.measure.marching_cubes and plyfile on the host; here the lattice never
leaves the GPU.  Rule, output order and measurements: DESIGN.md §3h; CPU restatement: tests/mc_restatement.py.

Parity with skimage's Lewiner variant is NOT pinned (skimage is absent from this environment): the vertex set is the same by construction (one
vertex per straddling lattice edge, linear interpolation), but on ambiguous configurations the triangulations may differ."""
import ctypes
import math
from typing import Optional, Tuple

import torch

from . import lib as L

DENSITY_THRE = 0.7          # the grid extraction's density mask: density > 0.7 (SampleGrid.query_dense, dreg_ngp_alpha_keep; sample_grid.py:186,328)
QUERY_CHUNK = 1 << 22       # lattice nodes per density query


def level_for_alpha(alpha: float = 0.7, delta: float = 1e-2) -> float:
    """The density at which the extraction's opacity 1 - exp(-delta * density) (SampleGrid._delta = 1e-2) reaches `alpha`: -ln(1 - alpha) / delta
    (120.4 for 0.7).  An alternative --mesh_level; the default is the density mask's own threshold."""
    return -math.log(1.0 - alpha) / delta


def marching_cubes(values: torch.Tensor, level: float, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)) -> Tuple[torch.Tensor, torch.Tensor]:
    """values fp32 [nz,ny,nx] on a GPU (x fastest; node (ix,iy,iz) at origin + i * spacing) -> (verts fp32 [V,3], faces int32 [F,3]) on the same
    device: the iso-surface value == level as an indexed mesh, inside = value > level, right-hand normals toward the lower values.  Two library
    calls with one host readback (V, F) between them; identical bytes between runs.  There is no CPU path."""
    if not values.is_cuda:
        raise ValueError("marching_cubes: values must be on a GPU (there is no CPU path)")
    if values.dim() != 3 or values.dtype != torch.float32:
        raise ValueError(f"marching_cubes: values {tuple(values.shape)} {values.dtype} must be fp32 [nz,ny,nx]")
    if len(origin) != 3 or len(spacing) != 3:
        raise ValueError("marching_cubes: origin and spacing take three numbers each")
    values = values.contiguous()
    nz, ny, nx = (int(v) for v in values.shape)
    lib = L.load()
    nbytes = int(lib.dreg_mc_workspace_bytes(nx, ny, nz))
    if nbytes == 0:
        raise ValueError(f"marching_cubes: lattice {nx} x {ny} x {nz}: every dimension must be in [2, 1024] and the nodes at most 2^28")
    dev = values.device
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        L.check(lib.dreg_mc_count(L.ptr(values), nx, ny, nz, float(level), L.ptr(ws), nbytes, L.ptr(counts), L.stream()), "dreg_mc_count")
        V, F = (int(v) for v in counts.tolist())               # the one host synchronisation: the outputs' sizes
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        org, spc = (L.c_float * 3)(*[float(v) for v in origin]), (L.c_float * 3)(*[float(v) for v in spacing])
        L.check(lib.dreg_mc_emit(L.ptr(values), nx, ny, nz, float(level), org, spc, L.ptr(ws), nbytes, L.ptr(verts) if V else None,
                                 L.ptr(faces) if F else None, V, F, L.stream()), "dreg_mc_emit")
    return verts, faces


def lattice_of(aabb, resolution: int):
    """(origin, spacing) as fp32-exact Python floats of the (resolution + 1)^3 node lattice that spans the aabb."""
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    lo, hi = [f32(v) for v in aabb[:3]], [f32(v) for v in aabb[3:]]
    spacing = [f32((torch.tensor(h, dtype=torch.float32) - torch.tensor(l, dtype=torch.float32)) / resolution) for l, h in zip(lo, hi)]
    return lo, spacing


@torch.no_grad()
def sample_density_lattice(field, resolution: int, chunk: int = QUERY_CHUNK) -> torch.Tensor:
    """The field's density at the (resolution + 1)^3 nodes spanning its aabb: fp32 [n,n,n] (z, y, x).  Node i of an axis is queried at
    lo + (float)i * spacing in fp32 — the position the mesh gives it — except the last one, queried at hi exactly: a node on an aabb face is not
    strictly inside (ngp_unit_cube), so the outer shell of the lattice is exactly 0 and every level > 0 gives a closed mesh."""
    dev = field.aabb.device
    aabb = field._aabb_host()
    n = resolution + 1
    origin, spacing = lattice_of(aabb, resolution)
    axes = []
    for c in range(3):
        a = torch.tensor(origin[c], dtype=torch.float32, device=dev) + torch.arange(n, dtype=torch.float32, device=dev) * torch.tensor(spacing[c], dtype=torch.float32, device=dev)
        a[-1] = aabb[3 + c]
        axes.append(a)
    out = torch.empty(n * n * n, dtype=torch.float32, device=dev)
    planes = max(1, chunk // (n * n))
    for z0 in range(0, n, planes):
        z1 = min(n, z0 + planes)
        Z, Y, X = torch.meshgrid(axes[2][z0:z1], axes[1], axes[0], indexing="ij")
        density, _ = field.query_raw(torch.stack([X, Y, Z], dim=-1).reshape(-1, 3))
        out[z0 * n * n:z1 * n * n] = density
    return out.view(n, n, n)


@torch.no_grad()
def block_mesh(field, resolution: int = 256, level: Optional[float] = None, normals: bool = True, colors: bool = True, chunk: int = QUERY_CHUNK) -> dict:
    """Surface mesh of a bounded block: density at the (resolution + 1)^3 nodes spanning the aabb (query_raw, in chunks), marching cubes at `level`,
    then per vertex the field's own normal (ngp.field_normals: -grad density, normalised) and the colour net's mean over the grid extraction's 18
    fixed viewing directions (query_rgb_mean).  Returns {"verts" fp32 [V,3], "faces" int32 [F,3], "normals" fp32 [V,3] or None, "colors" fp32
    [V,3] in [0,1] or None, "level", "origin", "spacing", "resolution"}.
    level defaults to DENSITY_THRE = 0.7, the grid extraction's density mask (density > 0.7): the mesh bounds the region voxel_mask keeps.  Whether
    that level gives the best-looking surface on trained scenes has not been measured (level_for_alpha(0.7) = 120.4, the density of opacity 0.7 over
    SampleGrid's delta, is the other candidate).  level must be > 0 for the mesh to be closed at the aabb faces."""
    if field.unbounded:
        raise NotImplementedError("block_mesh: the contracted (unbounded) field is not implemented (its lattice would live in contracted space)")
    if resolution < 1 or (resolution + 1) ** 3 > 1 << 28:
        raise ValueError(f"block_mesh: resolution {resolution} must be in [1, 644] (at most 2^28 lattice nodes)")
    from . import ngp
    level = DENSITY_THRE if level is None else float(level)
    values = sample_density_lattice(field, resolution, chunk)
    origin, spacing = lattice_of(field._aabb_host(), resolution)
    verts, faces = marching_cubes(values, level, origin, spacing)
    out = {"verts": verts, "faces": faces, "normals": None, "colors": None, "level": level, "origin": origin, "spacing": spacing, "resolution": resolution}
    if normals:
        out["normals"] = ngp.field_normals(field, verts) if verts.shape[0] else verts.new_zeros(0, 3)
    if colors:
        if verts.shape[0]:
            dirs = ngp.SampleGrid._generate_fixed_viewing_directions().to(verts.device).float().contiguous()
            rgb = verts.new_empty(verts.shape[0], 3)
            for a in range(0, verts.shape[0], chunk):
                _, raw = field.query_raw(verts[a:a + chunk])
                rgb[a:a + chunk] = field.query_rgb_mean(raw, dirs)
            out["colors"] = rgb
        else:
            out["colors"] = verts.new_zeros(0, 3)
    return out


def transform_mesh(verts: torch.Tensor, normals: Optional[torch.Tensor], pose: torch.Tensor):
    """Move a mesh by a rigid pose ([4,4] or [3,4], source -> target): verts -> R verts + t, normals -> R normals.  Faces are unchanged (a
    rotation keeps the winding)."""
    P = pose.detach().to(device=verts.device, dtype=verts.dtype).reshape(-1, 4)[:3]
    R, t = P[:, :3], P[:, 3]
    return verts @ R.T + t, (None if normals is None else normals @ R.T)


def merge_meshes(a: dict, b: dict) -> dict:
    """Two meshes as one: b's vertices follow a's and its face indices are offset by a's vertex count.  Normals / colours are kept when both
    have them."""
    out = {"verts": torch.cat([a["verts"], b["verts"]]), "faces": torch.cat([a["faces"], b["faces"] + a["verts"].shape[0]])}
    for k in ("normals", "colors"):
        out[k] = torch.cat([a[k], b[k]]) if a.get(k) is not None and b.get(k) is not None else None
    return out


def mesh_area_volume(verts: torch.Tensor, faces: torch.Tensor) -> Tuple[float, float]:
    """(surface area, enclosed volume) in fp64, plain torch.  The volume is the signed sum of the tetrahedra (origin, a, b, c): positive for a
    closed mesh whose right-hand normals point outward, meaningless for an open one."""
    v = verts.double()
    f = faces.long()
    if f.shape[0] == 0:
        return 0.0, 0.0
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1).sum()
    vol = (a * torch.linalg.cross(b, c)).sum() / 6.0
    return float(area), float(vol)


# ---------------------------------------------------------------------------------------------------------------- evaluator outputs
def write_block_mesh(ckpt_path: str, dev, resolution: int = 256, level: Optional[float] = None, path: Optional[str] = None, log=print) -> dict:
    """eval_ngp_nerf.py --mesh for one block: mesh.ply next to the checkpoint (or at `path`); prints V, F, area and volume.  Returns the mesh."""
    import os
    from . import vis_dump
    from .visibility import load_block
    field = load_block(ckpt_path, dev)[0]
    m = block_mesh(field, resolution, level)
    path = path or os.path.join(os.path.dirname(ckpt_path), "mesh.ply")
    vis_dump.write_mesh_ply(path, m["verts"].cpu().numpy(), m["faces"].cpu().numpy(), m["colors"].cpu().numpy(), m["normals"].cpu().numpy())
    area, vol = mesh_area_volume(m["verts"], m["faces"])
    log(f"{path}: level {m['level']:g}, resolution {resolution}: V {m['verts'].shape[0]}, F {m['faces'].shape[0]}, area {area:.4f}, volume {vol:.4f}")
    return m


def merged_scene_mesh(output_dir: str, src_path: str, tgt_path: str, pose_gt: torch.Tensor, pose_pred: torch.Tensor, dev, resolution: int = 256,
                      level: Optional[float] = None, mesher=None) -> dict:
    """eval_nerf_regtr.py --merged_mesh for one scene: the source block's mesh moved into the target frame by the predicted pose
    (merged_mesh_pred.ply) and by the known pose (merged_mesh_gt.ply), each concatenated with the target block's mesh (source vertices first, the
    target's face indices offset).  Poses are source -> target, [4,4] or [3,4], as --render_merged takes them.  mesher(path) -> mesh dict may be
    injected (tests).  Returns {"pred": mesh, "gt": mesh, "src": mesh, "tgt": mesh}."""
    import os
    from . import vis_dump
    if mesher is None:
        from .visibility import load_block

        def mesher(p):
            return block_mesh(load_block(p, dev)[0], resolution, level)
    src, tgt = mesher(src_path), mesher(tgt_path)
    os.makedirs(output_dir, exist_ok=True)
    out = {"src": src, "tgt": tgt}
    for name, P in (("pred", pose_pred), ("gt", pose_gt)):
        v, nrm = transform_mesh(src["verts"], src.get("normals"), P)
        m = merge_meshes({"verts": v, "faces": src["faces"], "normals": nrm, "colors": src.get("colors")}, tgt)
        cpu = lambda t: None if t is None else t.detach().cpu().numpy()
        vis_dump.write_mesh_ply(os.path.join(output_dir, f"merged_mesh_{name}.ply"), cpu(m["verts"]), cpu(m["faces"]), cpu(m["colors"]), cpu(m["normals"]))
        out[name] = m
    return out
