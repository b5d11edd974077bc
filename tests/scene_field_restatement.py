"""CPU restatement of the scene density field (csrc/scene_field.hip, dreg_nerf_amd/scene_field.py; rule: DESIGN.md §3k) in numpy: the K-block form of
tests/pair_field_restatement.py.  Everything that is a RULE is fp64 here (coverage, weights, blend); the one piece the kernel pins to fp32 bits,
the position of a scene-frame point in a block's frame, is restated in fp32 numpy ops in the kernel's order.  A block is a dict: roi (6 floats),
binary (bool / uint8 [rx,ry,rz]), center (3 floats) and sigma, a callable x [N,3] -> density [N] in the block's own frame."""
import numpy as np


def pose_f32(pose):
    """The fp64 pose ([3,4] or [4,4], block -> scene) rounded to fp32 once: (Rf [3,3], tf [3]); None stays None."""
    if pose is None:
        return None
    P = np.asarray(pose, dtype=np.float64).reshape(-1, 4)[:3]
    return P[:, :3].astype(np.float32), P[:, 3].astype(np.float32)


def to_block_f32(x, pose32):
    """x_b of the fp32 scene-frame points x [N,3]: d = x - tf, x_b[k] = (Rf[0][k] d[0] + Rf[1][k] d[1]) + Rf[2][k] d[2], every operation rounded to
    fp32 (numpy float32 arithmetic does not contract); without a pose x itself, the same bits."""
    x = np.asarray(x, dtype=np.float32)
    if pose32 is None:
        return x
    Rf, tf = pose32
    d = [x[:, k] - tf[k] for k in range(3)]
    return np.stack([(Rf[0, k] * d[0] + Rf[1, k] * d[1]) + Rf[2, k] * d[2] for k in range(3)], axis=1).astype(np.float32)


def to_block(x, pose):
    """The same map in fp64 from the fp64 pose: R^T (x - t); without a pose x."""
    x = np.asarray(x, dtype=np.float64)
    if pose is None:
        return x
    P = np.asarray(pose, dtype=np.float64).reshape(-1, 4)[:3]
    return (x - P[:, 3]) @ P[:, :3]


def covered(roi, binary, x, fp32=False):
    """Own coverage of a block at x [N,3] of its frame: u = (x - lo) / ext, inside iff 0 <= u <= 1 on all axes, cell clamp(floor(u res), 0, res - 1),
    binary != 0.  fp32=True evaluates u and u * res in float32 (the kernel's lookup)."""
    ft = np.float32 if fp32 else np.float64
    x = np.asarray(x, dtype=ft)
    roi = np.asarray(roi, dtype=ft)
    binary = np.asarray(binary)
    lo, ext = roi[:3], roi[3:] - roi[:3]
    u = (x - lo) / ext
    inside = ((u >= 0) & (u <= 1)).all(axis=1)
    res = np.asarray(binary.shape, dtype=ft)
    ci = np.clip(np.floor(np.where(inside[:, None], u, 0) * res), 0, res - 1).astype(np.int64)
    return inside & (binary[ci[:, 0], ci[:, 1], ci[:, 2]] != 0)


def deltas(xs, centers):
    """delta_b = |x_b - c_b|^2 + 1e-12, [N,K] fp64."""
    return np.stack([((np.asarray(x, dtype=np.float64) - np.asarray(c, dtype=np.float64)) ** 2).sum(axis=1) + 1e-12 for x, c in zip(xs, centers)], axis=1)


def weights(m, delta, power=4.0):
    """The overlap weights omega [N,K] from the coverages m [N,K] and delta [N,K], fp64.  C_b = the other covering blocks.  m_b = 0: 0; |C_b| = 0: 1;
    |C_b| = 1: omega_lo = 1 / (1 + (delta_lo / delta_hi)^(p/2)) and omega_hi = 1 - omega_lo; |C_b| >= 2: 1 / (1 + sum over b' in C_b, ascending,
    of (delta_b / delta_b')^(p/2))."""
    m = np.asarray(m, dtype=bool)
    N, K = m.shape
    hp = 0.5 * power
    om = np.zeros((N, K))
    for b in range(K):
        others = m.copy()
        others[:, b] = False
        cnt = others.sum(axis=1)
        total = np.zeros(N)
        for o in range(K):
            if o != b:
                total = total + np.where(others[:, o], (delta[:, b] / delta[:, o]) ** hp, 0.0)
        w = 1.0 / (1.0 + total)
        # the pair's form where exactly one LOWER block covers the point as well
        lower_one = (cnt == 1) & others[:, :b].any(axis=1)
        if lower_one.any():
            d_lo = np.where(others, delta, 0.0).sum(axis=1)                      # the one other block's delta
            w = np.where(lower_one, 1.0 - 1.0 / (1.0 + (np.where(lower_one, d_lo, 1.0) / delta[:, b]) ** hp), w)
        om[:, b] = np.where(m[:, b], w, 0.0)
    return om


def log_ratios(m, delta, power=4.0):
    """max over the covering pairs (b, b') of |y|, y = p/2 ln(delta_b / delta_b'), per point [N] (0 where fewer than two blocks cover): the exponents
    whose size bounds the weights' error."""
    m = np.asarray(m, dtype=bool)
    N, K = m.shape
    y = np.zeros(N)
    for b in range(K):
        for o in range(K):
            if o != b:
                y = np.maximum(y, np.where(m[:, b] & m[:, o], np.abs(0.5 * power * np.log(delta[:, b] / delta[:, o])), 0.0))
    return y


def scene_density(blocks, xs, power=4.0):
    """The scene density at points given in every block's frame (xs: K arrays [N,3]), fp64: {sigma [N], weight_block [N,K], sigma_block [N,K], m
    [N,K], delta [N,K]}.  sigma_block = m_b ? sigma_b(x_b) : 0; sigma = ((p_0 + p_1) + p_2) + p_3 with p_b = omega_b sigma_b."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    m = np.stack([covered(b["roi"], b["binary"], x) for b, x in zip(blocks, xs)], axis=1)
    delta = deltas(xs, [b["center"] for b in blocks])
    om = weights(m, delta, power)
    sb = np.stack([np.where(m[:, k], b["sigma"](x), 0.0) for k, (b, x) in enumerate(zip(blocks, xs))], axis=1)
    sigma = np.zeros(len(xs[0]))
    for k in range(len(blocks)):
        sigma = sigma + om[:, k] * sb[:, k]
    return {"sigma": sigma, "weight_block": om, "sigma_block": sb, "m": m, "delta": delta}


def vertex_attributes(weight_block, sigma_block, Rs, grads, colors):
    """Per-vertex blend (scene_field.blend_scene_attributes) in fp64, row by row: a_b = omega_b sigma_b; g = sum_b omega_b R_b grad_b (R_b None: the
    identity), normal = -g / |g| or zeros; colour = sum a_b c_b / sum a_b and share = a_b / sum a, zeros where the denominator is 0."""
    V, K = np.asarray(weight_block).shape
    nrm, col, share = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros((V, K))
    for i in range(V):
        g = np.zeros(3)
        for b in range(K):
            gb = np.asarray(grads[b][i], dtype=np.float64)
            g = g + float(weight_block[i][b]) * (gb if Rs[b] is None else np.asarray(Rs[b], dtype=np.float64) @ gb)
        n = np.sqrt((g * g).sum())
        if n > 0 and np.isfinite(n):
            nrm[i] = -g / n
        a = [float(weight_block[i][b]) * float(sigma_block[i][b]) for b in range(K)]
        if sum(a) > 0:
            col[i] = sum(a[b] * np.asarray(colors[b][i], dtype=np.float64) for b in range(K)) / sum(a)
            share[i] = np.asarray(a) / sum(a)
    return nrm, col, share
