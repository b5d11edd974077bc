"""CPU restatement of the merged voxel grid of a registered scene (csrc/scene_grid.hip, dreg_nerf_amd/scene_grid.py; rule: DESIGN.md §3l) in numpy, on
top of tests/scene_field_restatement.py.  Everything that is a RULE is fp64 here (the density through scene_field_restatement.scene_density, alpha /
keep, the colour blend with its single-carrier and non-finite rules, the zero rows); the one piece the kernel pins to fp32 bits, the sample position
of a cell, is restated in fp32 numpy ops in the kernel's order.  A block is scene_field_restatement's dict plus rgb, a callable x [N,3] -> the
block's mean colour [N,3] over the 18 fixed directions in the block's own frame."""
import numpy as np

import scene_field_restatement as SF


def cell_indices(res):
    """(x, y, z) int64 [n] of the flat indices f = (x ry + y) rz + z, f ascending."""
    rx, ry, rz = (int(v) for v in res)
    f = np.arange(rx * ry * rz, dtype=np.int64)
    return f // (ry * rz), (f // rz) % ry, f % rz


def sample_positions_f32(res, aabb, jitter=None):
    """w [n,3] fp32 of every cell: u_k = ((float)c_k + j_k) / (float)r_k, w_k = u_k (hi_k - lo_k) + lo_k, every operation rounded to fp32 (numpy
    float32 arithmetic does not contract); jitter [n,3] or None = 0.5 on every axis."""
    c = cell_indices(res)
    n = c[0].shape[0]
    box = np.asarray(aabb, dtype=np.float32)
    j = np.full((n, 3), 0.5, dtype=np.float32) if jitter is None else np.asarray(jitter, dtype=np.float32).reshape(n, 3)
    out = np.empty((n, 3), dtype=np.float32)
    for k in range(3):
        u = (c[k].astype(np.float32) + j[:, k]) / np.float32(res[k])
        out[:, k] = u * (box[3 + k] - box[k]) + box[k]
    return out


def alpha_keep(sigma, delta=1e-2, density_thre=0.7):
    """alpha = clip(1 - exp(-delta sigma), 0, 1), keep = sigma > density_thre (a NaN sigma is not kept)."""
    sigma = np.asarray(sigma, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.clip(1.0 - np.exp(-delta * sigma), 0.0, 1.0)
    return alpha, sigma > density_thre


def blend(a, c):
    """The colour of cells from their blocks' a_b = omega_b sigma_b [N,K] and mean colours c_b [N,K,3], row by row: (sum_b a_b c_b) / (sum_b a_b),
    both sums from block 0 upwards; exactly one block with a_b != 0: that block's c_b itself; the denominator or a product not finite: c_b of the
    block with the largest a_b, the lowest index on a tie; no block with a_b != 0: 0."""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    N, K = a.shape
    out = np.zeros((N, 3))
    for i in range(N):
        car = [b for b in range(K) if a[i, b] != 0]
        if not car:
            continue
        if len(car) == 1:
            out[i] = c[i, car[0]]
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            prods = [a[i, b] * c[i, b] for b in car]
            den = sum(a[i, b] for b in car)
        if not np.isfinite(den) or not all(np.isfinite(p).all() for p in prods):
            best = car[0]
            for b in car[1:]:
                if a[i, b] > a[i, best]:
                    best = b
            out[i] = c[i, best]
            continue
        num = np.zeros(3)
        for p in prods:
            num = num + p
        out[i] = num / den
    return out


def scene_grid(blocks, poses, res, aabb, jitter=None, power=4.0, delta=1e-2, density_thre=0.7):
    """The merged grid: {"w" fp32 [n,3], "sigma" [n], "alpha" [n], "keep" bool [n], "rgb" [n,3], "voxel_grid" [n,7] = (w | rgb | alpha) at kept
    cells and exactly 0 at all others, "voxel_mask" int64 ascending, "parts": scene_field_restatement.scene_density's dict}.  poses: the fp64
    poses (block -> scene) or None per block; the cells reach every block through the fp32 pose, as the kernel's do."""
    w = sample_positions_f32(res, aabb, jitter)
    xs = [SF.to_block_f32(w, SF.pose_f32(p)) for p in poses]
    parts = SF.scene_density(blocks, xs, power)
    sigma = parts["sigma"]
    alpha, keep = alpha_keep(sigma, delta, density_thre)
    a = parts["weight_block"] * parts["sigma_block"]
    rgb = np.zeros((w.shape[0], 3))
    idx = np.nonzero(keep)[0]
    if idx.size:
        c = np.stack([np.asarray(b["rgb"](x[idx]), dtype=np.float64) for b, x in zip(blocks, xs)], axis=1)
        rgb[idx] = blend(a[idx], c)
    grid = np.zeros((w.shape[0], 7))
    grid[idx, :3] = w[idx]
    grid[idx, 3:6] = rgb[idx]
    grid[idx, 6] = alpha[idx]
    return {"w": w, "sigma": sigma, "alpha": alpha, "keep": keep, "rgb": rgb, "voxel_grid": grid, "voxel_mask": idx.astype(np.int64), "parts": parts}
