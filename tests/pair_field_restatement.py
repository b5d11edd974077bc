"""CPU restatement of the pair density field (dreg_pair_density of csrc/scene_field.hip, dreg_nerf_amd/pair_field.py; rule: DESIGN.md §3i) in numpy.  Everything that is a
RULE is fp64 here (coverage, weight, blend); the one piece the kernel pins to fp32 bits, the position of a point in the source frame, is restated in
fp32 numpy ops in the kernel's order.  A block is a dict: roi (6 floats), binary (bool / uint8 [rx,ry,rz]), center (3 floats) and sigma, a
callable x [N,3] -> density [N] in the block's own frame."""
import numpy as np


def pose_f32(pose):
    """The fp64 pose ([3,4] or [4,4]) rounded to fp32 once: (Rf [3,3], tf [3])."""
    P = np.asarray(pose, dtype=np.float64).reshape(-1, 4)[:3]
    return P[:, :3].astype(np.float32), P[:, 3].astype(np.float32)


def to_source_f32(x, Rf, tf):
    """x_S of the fp32 points x [N,3] (target frame): d = x - tf, x_S[k] = (Rf[0][k] d[0] + Rf[1][k] d[1]) + Rf[2][k] d[2], every operation rounded
    to fp32 (numpy float32 arithmetic does not contract)."""
    x = np.asarray(x, dtype=np.float32)
    d = [x[:, k] - tf[k] for k in range(3)]
    return np.stack([(Rf[0, k] * d[0] + Rf[1, k] * d[1]) + Rf[2, k] * d[2] for k in range(3)], axis=1).astype(np.float32)


def to_source(x, pose):
    """The same map in fp64 from the fp64 pose: R^T (x - t)."""
    P = np.asarray(pose, dtype=np.float64).reshape(-1, 4)[:3]
    return (np.asarray(x, dtype=np.float64) - P[:, 3]) @ P[:, :3]


def covered(roi, binary, x, fp32=False):
    """Own coverage of a block at x [N,3] of its frame: u = (x - lo) / ext, inside iff 0 <= u <= 1 on all axes, cell clamp(floor(u res), 0, res - 1),
    binary != 0.  fp32=True evaluates u and u * res in float32 (the kernel's lookup: a point within rounding of a cell face lands where the kernel
    puts it)."""
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


def weight(x_s, x_t, c_s, c_t, power=4.0):
    """The source's overlap weight where both blocks cover the point: q = (|x_S - c_S|^2 + 1e-12) / (|x_T - c_T|^2 + 1e-12), w = 1 / (1 + q^(p/2)), fp64."""
    ds = ((np.asarray(x_s, dtype=np.float64) - np.asarray(c_s, dtype=np.float64)) ** 2).sum(axis=1)
    dt = ((np.asarray(x_t, dtype=np.float64) - np.asarray(c_t, dtype=np.float64)) ** 2).sum(axis=1)
    q = (ds + 1e-12) / (dt + 1e-12)
    return 1.0 / (1.0 + q ** (0.5 * power))


def log_ratio(x_s, x_t, c_s, c_t, power=4.0):
    """y = 0.5 p ln q of the same q (the exponent whose size bounds the weight's error)."""
    ds = ((np.asarray(x_s, dtype=np.float64) - np.asarray(c_s, dtype=np.float64)) ** 2).sum(axis=1)
    dt = ((np.asarray(x_t, dtype=np.float64) - np.asarray(c_t, dtype=np.float64)) ** 2).sum(axis=1)
    return 0.5 * power * np.log((ds + 1e-12) / (dt + 1e-12))


def block_weights(m_s, m_t, w):
    """w_S = m_S ? (m_T ? w : 1) : 0,  w_T = m_T ? (m_S ? 1 - w : 1) : 0."""
    w_s = np.where(m_s, np.where(m_t, w, 1.0), 0.0)
    w_t = np.where(m_t, np.where(m_s, 1.0 - w, 1.0), 0.0)
    return w_s, w_t


def pair_density(src, tgt, x_s, x_t, power=4.0):
    """The pair density at points given in both frames (x_s [N,3] source, x_t [N,3] target), fp64: {sigma, w_src, w_tgt, sigma_src, sigma_tgt, m_src,
    m_tgt}.  sigma_b = m_b ? sigma_b(x_b) : 0; sigma = w_S sigma_S + w_T sigma_T."""
    x_s, x_t = np.asarray(x_s, dtype=np.float64), np.asarray(x_t, dtype=np.float64)
    m_s, m_t = covered(src["roi"], src["binary"], x_s), covered(tgt["roi"], tgt["binary"], x_t)
    w_s, w_t = block_weights(m_s, m_t, weight(x_s, x_t, src["center"], tgt["center"], power))
    s_s = np.where(m_s, src["sigma"](x_s), 0.0)
    s_t = np.where(m_t, tgt["sigma"](x_t), 0.0)
    return {"sigma": w_s * s_s + w_t * s_t, "w_src": w_s, "w_tgt": w_t, "sigma_src": s_s, "sigma_tgt": s_t, "m_src": m_s, "m_tgt": m_t}


def vertex_attributes(w_s, w_t, s_s, s_t, R, g_s, g_t, c_s, c_t):
    """Per-vertex blend (pair_field.blend_vertex_attributes) in fp64, row by row: a_b = w_b sigma_b; g = w_S R grad_S + w_T grad_T, normal = -g / |g| or
    zeros; colour = (a_S c_S + a_T c_T) / (a_S + a_T) and weight_src = a_S / (a_S + a_T), zeros where the denominator is 0."""
    R = np.asarray(R, dtype=np.float64)
    V = len(w_s)
    nrm, col, wsrc = np.zeros((V, 3)), np.zeros((V, 3)), np.zeros(V)
    for i in range(V):
        g = w_s[i] * (R @ np.asarray(g_s[i], dtype=np.float64)) + w_t[i] * np.asarray(g_t[i], dtype=np.float64)
        n = np.sqrt((g * g).sum())
        if n > 0 and np.isfinite(n):
            nrm[i] = -g / n
        a_s, a_t = float(w_s[i]) * float(s_s[i]), float(w_t[i]) * float(s_t[i])
        if a_s + a_t > 0:
            col[i] = (a_s * np.asarray(c_s[i], dtype=np.float64) + a_t * np.asarray(c_t[i], dtype=np.float64)) / (a_s + a_t)
            wsrc[i] = a_s / (a_s + a_t)
    return nrm, col, wsrc
