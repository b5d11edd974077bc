"""fp64 restatement (numpy) of the density gradient of csrc/ngp_grad.hip: the straight-through gradient of the hash-grid density
field, the fp16 roundings of the forward taken as identity.

For a point x inside the aabb (lo, hi), u = (x - lo) / (hi - lo); per level l with scale s_l: pos = u s_l + 1/2, cell g = floor(pos), w = pos - g;
the level's two features are the trilinear interpolation of the table entries at the cell's 8 corners (index: dense x + y res + z res^2 or the
hash x ^ y 2654435761 ^ z 805459861, modulo the level's size).  hidden = relu(W1 enc), logit = W2[0] . hidden, sigma = exp(logit - 1).

    g_j = W2[0][j] where hidden unit j is active (the ReLU mask: an INPUT here), else 0;   f_i = sum_j W1[j][i] g_j
    d enc_{2l+k} / d u_c = s_l sum_corners sgn_c w_a w_b table[corner][k]     (sgn_c = +-1 by the corner's side on axis c; a, b the other axes)
    du_c = sum_l sum_k f_{2l+k} d enc_{2l+k} / d u_c;        grad_c = sigma du_c / (hi_c - lo_c), zero where x is not strictly inside the aabb.

coords = np.float32: u, pos and w are formed in fp32 exactly as the field forms them (they decide the cell: part of the field's definition), everything
after them in fp64 — what the kernel is held to.  coords = np.float64: the whole chain in fp64, consistent with forward64 (the finite-difference test).
The level table is an input: dicts of arrays offset, size, res, scale, hashed (any number of levels)."""
import numpy as np

P1, P2 = np.uint32(2654435761), np.uint32(805459861)


def levels_from_ctypes(arrs):
    """The five 16-entry arrays of dreg_ngp_level_table (NGPradianceField._levels) as a dict of numpy arrays."""
    offset, size, res, scale, hashed = (np.array(list(a)) for a in arrs)
    return {"offset": offset.astype(np.int64), "size": size.astype(np.uint32), "res": res.astype(np.uint32), "scale": scale.astype(np.float32),
            "hashed": hashed.astype(np.uint32)}


def grid_index(cx, cy, cz, res, size, hashed):
    cx, cy, cz = cx.astype(np.uint32), cy.astype(np.uint32), cz.astype(np.uint32)
    with np.errstate(over="ignore"):
        idx = (cx ^ (cy * P1) ^ (cz * P2)) if hashed else (cx + cy * np.uint32(res) + cz * np.uint32(res) * np.uint32(res))
    return (idx % np.uint32(size)).astype(np.int64)


def unit_cube(x, aabb, coords):
    """u (clamped to [0,1]) and the strictly-inside flag, in the arithmetic `coords`."""
    x = np.asarray(x).astype(coords)                   # fp32 points are exact in either arithmetic; fp64 points (finite differences) stay fp64
    lo, hi = np.asarray(aabb[:3], dtype=np.float32).astype(coords), np.asarray(aabb[3:], dtype=np.float32).astype(coords)
    u = ((x - lo) / (hi - lo)).astype(coords)
    inside = ((u > 0) & (u < 1)).all(axis=1)
    return np.clip(u, 0, 1).astype(coords), inside


def level_cells(u, scale, coords):
    """g (uint32 [N,3]) and w ([N,3], as fp64 values of the `coords` arithmetic) of one level."""
    pos = ((u * coords(scale)).astype(coords) + coords(0.5)).astype(coords)
    fl = np.floor(pos)
    return fl.astype(np.uint32), (pos - fl).astype(np.float64)


def _corners(g, w, lv, l, table):
    """Per corner: (table entries fp64 [N,2], per-axis weights [N,3], signs [3])."""
    t = np.asarray(table).reshape(-1, 2)                # gathered first, widened after: the table of a real block has 6 M entries
    for corner in range(8):
        b = [(corner >> c) & 1 for c in range(3)]
        idx = grid_index(g[:, 0] + np.uint32(b[0]), g[:, 1] + np.uint32(b[1]), g[:, 2] + np.uint32(b[2]), lv["res"][l], lv["size"][l], lv["hashed"][l])
        wa = np.stack([w[:, c] if b[c] else 1.0 - w[:, c] for c in range(3)], axis=1)
        yield t[int(lv["offset"][l]) + idx].astype(np.float64), wa, [1.0 if b[c] else -1.0 for c in range(3)]


def encode(x, table, lv, aabb, coords=np.float64):
    """enc fp64 [N, 2 L] (unrounded) and the inside flag."""
    u, inside = unit_cube(x, aabb, coords)
    nl = len(lv["scale"])
    enc = np.zeros((len(u), 2 * nl))
    for l in range(nl):
        g, w = level_cells(u, lv["scale"][l], coords)
        for t, wa, _ in _corners(g, w, lv, l, table):
            enc[:, 2 * l:2 * l + 2] += (wa[:, 0] * wa[:, 1] * wa[:, 2])[:, None] * t
    return enc, inside


def forward64(x, table, w1, w2, lv, aabb):
    """The unrounded fp64 forward: (sigma [N], mask bool [N,H], pre-activations [N,H])."""
    enc, inside = encode(x, table, lv, aabb, np.float64)
    pre = enc @ np.asarray(w1, dtype=np.float64).T
    logit = np.maximum(pre, 0.0) @ np.asarray(w2, dtype=np.float64)[0]
    return np.exp(logit - 1.0) * inside, pre > 0, pre


def mask_bits(mask_u64, n_hidden=64):
    """uint64 [N] -> bool [N, n_hidden]."""
    m = np.asarray(mask_u64).astype(np.uint64)
    return ((m[:, None] >> np.arange(n_hidden, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool)


def density_grad(x, table, w1, w2, lv, aabb, sigma, mask, coords=np.float32):
    """grad fp64 [N,3] and M [N,3] = the same sum with every term replaced by its absolute value (the scale of the rounding bound).
    sigma [N]: the density the gradient is scaled by (the device's own for the kernel tests); mask bool [N,H]."""
    w1, w2 = np.asarray(w1, dtype=np.float64), np.asarray(w2, dtype=np.float64)
    gj = np.where(mask, w2[0][None], 0.0)                                   # [N,H]
    f = gj @ w1                                                             # [N, 2L]
    fabs = np.abs(gj) @ np.abs(w1)
    u, inside = unit_cube(x, aabb, coords)
    nl = len(lv["scale"])
    du, dua = np.zeros((len(u), 3)), np.zeros((len(u), 3))
    for l in range(nl):
        g, w = level_cells(u, lv["scale"][l], coords)
        s = float(lv["scale"][l])
        for t, wa, sg in _corners(g, w, lv, l, table):
            v = f[:, 2 * l] * t[:, 0] + f[:, 2 * l + 1] * t[:, 1]
            va = fabs[:, 2 * l] * np.abs(t[:, 0]) + fabs[:, 2 * l + 1] * np.abs(t[:, 1])
            for c in range(3):
                a, b = (c + 1) % 3, (c + 2) % 3
                du[:, c] += s * sg[c] * wa[:, a] * wa[:, b] * v
                dua[:, c] += s * wa[:, a] * wa[:, b] * va
    ext = np.asarray(aabb[3:], dtype=np.float32).astype(np.float64) - np.asarray(aabb[:3], dtype=np.float32).astype(np.float64)
    sig = np.asarray(sigma, dtype=np.float64)[:, None] * inside[:, None]
    return sig * du / ext, np.abs(sig) * dua / ext


def face_distance(x, lv, aabb):
    """Smallest distance in world units, along any axis, from x to a cell face of any level: the finite-difference test keeps the points whose
    distance exceeds its step."""
    u, _ = unit_cube(x, aabb, np.float64)
    ext = (np.asarray(aabb[3:], dtype=np.float64) - np.asarray(aabb[:3], dtype=np.float64))
    d = np.full(len(u), np.inf)
    for s in lv["scale"]:
        pos = u * float(s) + 0.5
        fr = pos - np.floor(pos)
        d = np.minimum(d, (np.minimum(fr, 1.0 - fr) / float(s) * ext).min(axis=1))
    return d
