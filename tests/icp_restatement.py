"""fp64 restatement (numpy) of the point-to-plane ICP rule of csrc/icp.hip, with a brute-force nearest-neighbour search.

One iteration, for a pose (R, t) held in fp64 and rounded to fp32 where the kernel rounds it:
  q = R p + t;  the correspondence of p is the target point with the smallest squared distance, ties to the smallest (cell id, caller index);
  it counts iff d^2 <= max_dist^2 and its normal n is not the zero vector;  e = n.(q - p_t), J = [q x n, n];
  A = sum J^T J, b = sum J^T e;  Cholesky of A with pivots d_k^2: status 3 when d_k^2 <= eps_cond A_kk, status 2 when count < 6;
  xi = (omega, v) = -A^-1 b;  R <- exp(omega) R, t <- exp(omega) t + v;  status 1 when |omega| < tol_rot and |v| < tol_trans.
Everything after the fp32 rounding of the pose is fp64 here; the kernel forms q, e, J and d^2 in fp32 (the tests bound that difference)."""
import math

import numpy as np

NSUM = 30


def exp_so3(w):
    """Rodrigues: I + sin(th)/th K + (1 - cos th)/th^2 K^2, the second coefficient as (sin(th/2)/(th/2))^2 / 2."""
    w = np.asarray(w, dtype=np.float64)
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    a, c = 1.0, 0.5
    if th > 0.0:
        a = math.sin(th) / th
        h = math.sin(0.5 * th) / (0.5 * th)
        c = 0.5 * h * h
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * K + c * (K @ K)


def grid_of(points, cell):
    """lo, dims and per-point cell ids of TargetIndex, in fp32 as it forms them (cell doubled while the grid has more than 2^24 cells)."""
    points = np.asarray(points, dtype=np.float32)
    cell = np.float32(cell)
    mn, mx = points.min(axis=0), points.max(axis=0)
    while True:
        lo = (mn - cell).astype(np.float32)
        dims = [int(v) + 2 for v in np.floor(((mx - lo).astype(np.float32) / cell).astype(np.float32))]
        if dims[0] * dims[1] * dims[2] <= 1 << 24:
            break
        cell = np.float32(cell * np.float32(2))
    key = np.floor((((points - lo).astype(np.float32)) / cell).astype(np.float32)).astype(np.int64)
    cid = key[:, 0] + dims[0] * (key[:, 1] + dims[1] * key[:, 2])
    return lo, float(cell), tuple(dims), cid


def pose32(pose12):
    p = np.asarray(pose12, dtype=np.float64).astype(np.float32).astype(np.float64)
    return p[:9].reshape(3, 3), p[9:]


def transform(src, pose12):
    R, t = pose32(pose12)
    return np.asarray(src, dtype=np.float64) @ R.T + t


def nearest(src, tgt, cell_id, pose12, chunk=512):
    """Brute force: per source point the index of the nearest target point (ties: smallest (cell id, caller index)), its squared distance, and the
    squared distance of the runner-up (inf with one target point)."""
    q = transform(src, pose12)
    tgt = np.asarray(tgt, dtype=np.float64)
    order = np.lexsort((np.arange(len(tgt)), np.asarray(cell_id)))       # ascending (cell id, index): argmin takes the first minimum
    ts = tgt[order]
    best = np.empty(len(q), dtype=np.int64)
    d_best = np.empty(len(q))
    d_second = np.full(len(q), np.inf)
    for a in range(0, len(q), chunk):
        r = q[a:a + chunk, None, :] - ts[None]
        d2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        j = np.argmin(d2, axis=1)
        rows = np.arange(len(j))
        best[a:a + chunk] = order[j]
        d_best[a:a + chunk] = d2[rows, j]
        if ts.shape[0] > 1:
            d2[rows, j] = np.inf
            d_second[a:a + chunk] = d2.min(axis=1)
    return best, d_best, d_second


def correspondences(src, tgt, nrm, cell_id, pose12, max_dist):
    """corr int [Ns] (-1 = none) and dist2 fp64 [Ns] (inf for none)."""
    best, d_best, _ = nearest(src, tgt, cell_id, pose12)
    md2 = float(np.float32(max_dist) * np.float32(max_dist))
    n = np.asarray(nrm, dtype=np.float64)[best]
    ok = (d_best <= md2) & ~((n == 0.0).all(axis=1))
    return np.where(ok, best, -1), np.where(ok, d_best, np.inf)


def residuals(src, tgt, nrm, corr, pose12):
    """e [M], J [M,6], d2 [M] of the rows with a correspondence."""
    keep = corr >= 0
    q = transform(src, pose12)[keep]
    pt = np.asarray(tgt, dtype=np.float64)[corr[keep]]
    n = np.asarray(nrm, dtype=np.float64)[corr[keep]]
    r = q - pt
    e = (n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]
    J = np.concatenate([np.cross(q, n), n], axis=1)
    d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    return e, J, d2


def sums_given(src, tgt, nrm, corr, pose12):
    """The 30 sums for given correspondences: 21 of J^T J (upper triangle, row-major), 6 of J^T e, sum e^2, sum d^2, count."""
    e, J, d2 = residuals(src, tgt, nrm, corr, pose12)
    out = []
    for a in range(6):
        for b in range(a, 6):
            out.append(math.fsum(J[:, a] * J[:, b]))
    for a in range(6):
        out.append(math.fsum(J[:, a] * e))
    out += [math.fsum(e * e), math.fsum(d2), float(len(e))]
    return np.array(out)


def solve(S, pose12, tol_rot=1e-7, tol_trans=1e-7, eps_cond=1e-6):
    """One solve: (new pose12, stats row).  Status 2 / 3 return pose12 itself."""
    pose12 = np.asarray(pose12, dtype=np.float64)
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = S[k]
            k += 1
    b = np.asarray(S[21:27], dtype=np.float64)
    count = S[29]
    status, ratio, nw, nv = 0, 0.0, 0.0, 0.0
    Lc = np.zeros((6, 6))
    if count < 6:
        status = 2
    else:
        ratio = math.inf
        for c in range(6):
            d = A[c, c]
            for j in range(c):
                d -= Lc[c, j] * Lc[c, j]
            rt = d / A[c, c] if A[c, c] > 0 else 0.0
            ratio = min(ratio, rt)
            if not (A[c, c] > 0) or not (d > eps_cond * A[c, c]):
                status = 3
                break
            Lc[c, c] = math.sqrt(d)
            for i in range(c + 1, 6):
                v = A[i, c]
                for j in range(c):
                    v -= Lc[i, j] * Lc[c, j]
                Lc[i, c] = v / Lc[c, c]
    new = pose12
    if status == 0:
        y = np.zeros(6)
        xi = np.zeros(6)
        for i in range(6):
            v = -b[i]
            for j in range(i):
                v -= Lc[i, j] * y[j]
            y[i] = v / Lc[i, i]
        for i in range(5, -1, -1):
            v = y[i]
            for j in range(i + 1, 6):
                v -= Lc[j, i] * xi[j]
            xi[i] = v / Lc[i, i]
        nw = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
        nv = math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])
        E = exp_so3(xi[:3])
        R, t = pose12[:9].reshape(3, 3), pose12[9:]
        new = np.concatenate([(E @ R).reshape(9), E @ t + xi[3:]])
        if nw < tol_rot and nv < tol_trans:
            status = 1
    return new, np.array([count, S[27], S[28], nw, nv, ratio, float(status)])


def sums_kernel_arithmetic(src, tgt, nrm, cell_id, pose12, max_dist):
    """The 30 sums with q, d^2, e and J formed in fp32 in the kernel's operation order (numpy fp32 is IEEE, no contraction), brute-force search,
    fp64 sums: what the device computes up to the order of its fp64 additions.  Used to see the fp32 floor of a run on the CPU."""
    f = np.float32
    P = np.asarray(pose12, dtype=np.float64).astype(f)
    p = np.asarray(src, dtype=f)
    q = np.stack([((P[3 * c] * p[:, 0] + P[3 * c + 1] * p[:, 1]) + P[3 * c + 2] * p[:, 2]) + P[9 + c] for c in range(3)], axis=1)
    order = np.lexsort((np.arange(len(tgt)), np.asarray(cell_id)))
    ts = np.asarray(tgt, dtype=f)[order]
    ns = np.asarray(nrm, dtype=f)[order]
    best = np.empty(len(q), dtype=np.int64)
    bd = np.empty(len(q), dtype=f)
    for a in range(0, len(q), 512):
        r = q[a:a + 512, None, :] - ts[None]
        d2 = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
        j = np.argmin(d2, axis=1)
        best[a:a + 512] = j
        bd[a:a + 512] = d2[np.arange(len(j)), j]
    n = ns[best]
    ok = (bd <= f(max_dist) * f(max_dist)) & ~((n == 0).all(axis=1))
    q, n, r, bd = q[ok], n[ok], (q - ts[best])[ok], bd[ok]
    e = ((n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]).astype(np.float64)
    J = np.stack([q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2], q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2]], axis=1).astype(np.float64)
    out = [math.fsum(J[:, a] * J[:, b]) for a in range(6) for b in range(a, 6)] + [math.fsum(J[:, a] * e) for a in range(6)]
    return np.array(out + [math.fsum(e * e), math.fsum(bd.astype(np.float64)), float(len(e))])


def refine(src, tgt, nrm, pose12, max_dist, iters, cell=None, tol_rot=1e-7, tol_trans=1e-7, eps_cond=1e-6, kernel_arithmetic=False):
    """The whole run: (pose12, stats [iters,7]); rows after a freeze repeat the freezing row."""
    _, _, _, cid = grid_of(tgt, max_dist if cell is None else cell)
    pose12 = np.asarray(pose12, dtype=np.float64)
    rows = []
    for _ in range(iters):
        if rows and rows[-1][6] != 0:
            rows.append(rows[-1].copy())
            continue
        if kernel_arithmetic:
            S = sums_kernel_arithmetic(src, tgt, nrm, cid, pose12, max_dist)
        else:
            corr, _ = correspondences(src, tgt, nrm, cid, pose12, max_dist)
            S = sums_given(src, tgt, nrm, corr, pose12)
        pose12, row = solve(S, pose12, tol_rot, tol_trans, eps_cond)
        rows.append(row)
    return pose12, np.array(rows).reshape(iters, 7)


def pose12_of(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)])


def rre_deg(R_est, R_gt):
    c = (np.trace(np.asarray(R_est) @ np.asarray(R_gt).T) - 1.0) / 2.0
    # acos loses everything near 0: use the chord, |R_est - R_gt|_F = 2 sqrt(2) sin(th / 2)
    s = np.linalg.norm(np.asarray(R_est) - np.asarray(R_gt)) / (2.0 * math.sqrt(2.0))
    return math.degrees(2.0 * math.asin(min(1.0, s))) if c > -1 else 180.0


def rte(t_est, t_gt):
    return float(np.linalg.norm(np.asarray(t_est) - np.asarray(t_gt)))
