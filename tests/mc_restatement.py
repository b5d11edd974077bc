"""CPU restatement of the marching-cubes rule of csrc/marching_cubes.hip in numpy, and table-free invariants of a mesh.

marching_cubes(values, level, origin, spacing, fp32=False): the same classification, vertex rule and output order as the kernels.  fp64 by
default; fp32=True performs the five vertex operations in fp32 in the kernel's order (numpy rounds each fp32 operation once, as the device
does with contraction off).  The triangle table is read from the built library through dreg_mc_table (a host function: no GPU is needed)."""
import ctypes
import os

import numpy as np

_TABLE = None


def load_table():
    """(tris int8 [256, 3 * width], width) from the library."""
    global _TABLE
    if _TABLE is None:
        from dreg_nerf_amd import lib as L
        if not os.path.exists(L.LIB_PATH):
            from dreg_nerf_amd import build
            build.build(verbose=False)
        lib = L.load()
        w = ctypes.c_int(0)
        assert lib.dreg_mc_table(None, ctypes.byref(w)) == 0 and 1 <= w.value <= 16
        buf = np.zeros((256, 3 * w.value), dtype=np.int8)
        assert lib.dreg_mc_table(buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(w)) == 0
        _TABLE = (buf, int(w.value))
    return _TABLE


def edge_owner(e):
    """(dx, dy, dz, axis) of cube edge id e = 4 * axis + k: offset of the owning node from the cell's lowest node."""
    axis, k = e >> 2, e & 3
    a, b = k & 1, k >> 1
    return ((0, a, b), (a, 0, b), (a, b, 0))[axis] + (axis,)


def inside_mask(values, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(values) > level                     # NaN > level is False: NaN counts as outside


def edge_flags(ins):
    """flags bool [nz, ny, nx, 3]: the node's +x, +y, +z edge crosses."""
    f = np.zeros(ins.shape + (3,), dtype=bool)
    f[:, :, :-1, 0] = ins[:, :, :-1] != ins[:, :, 1:]
    f[:, :-1, :, 1] = ins[:, :-1, :] != ins[:, 1:, :]
    f[:-1, :, :, 2] = ins[:-1, :, :] != ins[1:, :, :]
    return f


def marching_cubes(values, level, origin, spacing, fp32=False, table=None):
    """values [nz, ny, nx] -> (verts [V,3] float64 or float32, faces [F,3] int32)."""
    tris, width = table if table is not None else load_table()
    ft = np.float32 if fp32 else np.float64
    vals = np.asarray(values, dtype=np.float32)
    nz, ny, nx = vals.shape
    ins = inside_mask(vals, np.float32(level))
    flags = edge_flags(ins)
    index = (np.cumsum(flags.reshape(-1)) - flags.reshape(-1)).reshape(nz, ny, nx, 3)       # exclusive prefix in (node, axis) order
    v = vals.astype(ft)
    lev, org, spc = ft(level), np.asarray(origin, dtype=np.float32).astype(ft), np.asarray(spacing, dtype=np.float32).astype(ft)
    iz, iy, ix, ax = np.nonzero(flags)                        # C order: ascending node, then axis
    node = np.stack([ix, iy, iz], axis=1)
    q = node.copy()
    q[np.arange(len(ax)), ax] += 1
    vp, vq = v[iz, iy, ix], v[q[:, 2], q[:, 1], q[:, 0]]
    with np.errstate(all="ignore"):
        t = (lev - vp) / (vq - vp)
        t = np.where(np.isfinite(t) & (t >= 0) & (t <= 1), t, ft(0.5)).astype(ft)
        verts = np.empty((len(ax), 3), dtype=ft)
        for c in range(3):
            along = org[c] + (node[:, c].astype(ft) + t) * spc[c]
            plain = org[c] + node[:, c].astype(ft) * spc[c]
            verts[:, c] = np.where(ax == c, along, plain)
    # faces: cells in ascending order of their lowest node, table order inside a cell
    cfg = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, c >> 1 & 1, c >> 2 & 1
        cfg |= ins[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int64) << c
    row = tris[cfg]                                           # [cz, cy, cx, 3 * width]
    faces = np.zeros(cfg.shape + (width, 3), dtype=np.int64)
    valid = (row.reshape(cfg.shape + (width, 3))[..., 0] >= 0)
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    for e in range(12):
        dx, dy, dz, axis = edge_owner(e)
        idx = index[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx, axis]
        sel = row.reshape(cfg.shape + (width, 3)) == e
        faces = np.where(sel, idx[..., None, None], faces)
    return verts, faces[valid].astype(np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------- table-free invariants
def directed_edge_counts(faces):
    """{(a, b): times the directed edge a -> b occurs}."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(uniq, cnt)}


def unmatched_edges(faces):
    """Directed edges that break "every directed edge occurs once and its reverse occurs once": [(a, b, count, reverse count)]."""
    d = directed_edge_counts(faces)
    return [(a, b, c, d.get((b, a), 0)) for (a, b), c in d.items() if c != 1 or d.get((b, a), 0) != 1]


def is_closed(faces):
    return not unmatched_edges(faces)


def repeated_index_faces(faces):
    f = np.asarray(faces).reshape(-1, 3)
    return int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())


def euler_characteristic(n_verts, faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return int(n_verts) - len(np.unique(e, axis=0)) + len(f)


def signed_volume(verts, faces):
    """Volume enclosed by a closed mesh whose right-hand normals point outward (fp64)."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def straddling_edge_count(values, level):
    return int(edge_flags(inside_mask(np.asarray(values, dtype=np.float32), np.float32(level))).sum())


def vertices_on_straddling_edges(verts, values, level, origin, spacing):
    """True when every vertex lies on a lattice edge whose two ends are on different sides of the level: two of its lattice coordinates are
    integers (to 1e-6 cells) and the edge that contains the third straddles.  A vertex that coincides with a node (t = 0 or 1 exactly) passes
    when any lattice edge at that node straddles."""
    vals = np.asarray(values, dtype=np.float32)
    nz, ny, nx = vals.shape
    flags = edge_flags(inside_mask(vals, np.float32(level)))
    g = (np.asarray(verts, dtype=np.float64) - np.asarray(origin, dtype=np.float64)) / np.asarray(spacing, dtype=np.float64)
    r = np.round(g)
    on = np.abs(g - r) < 1e-6
    if not (on.sum(axis=1) >= 2).all() or (r < 0).any() or (r > np.array([nx, ny, nz]) - 1).any():
        return False
    r = r.astype(np.int64)
    edge = on.sum(axis=1) == 2
    axis = np.argmin(on[edge], axis=1)
    node = r[edge]
    node[np.arange(len(axis)), axis] = np.floor(g[edge][np.arange(len(axis)), axis]).astype(np.int64)
    if not flags[node[:, 2], node[:, 1], node[:, 0], axis].all():
        return False
    for x, y, z in r[~edge]:
        near = [flags[z, y, x, a] for a in range(3)]
        near += [flags[z, y, x - 1, 0] if x > 0 else False, flags[z, y - 1, x, 1] if y > 0 else False, flags[z - 1, y, x, 2] if z > 0 else False]
        if not any(near):
            return False
    return True
