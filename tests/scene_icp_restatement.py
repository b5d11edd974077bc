"""fp64 restatement (numpy) of the joint K-block point-to-plane ICP of csrc/icp_scene.hip, over the functions of
tests/icp_restatement.py.

Poses G_b (12 numbers: R row-major, then t) map block b's frame to the anchor's (block 0, never moved).  One iteration:
  rel[i][j] = G_j^-1 G_i:  R_ij = R_j^T R_i, t_ij = R_j^T (t_i - t_j), every 3-term sum as (a0 b0 + a1 b1) + a2 b2;
  per enabled ordered pair (i, j), i != j:  S_ij = the 30 sums of the pair rule (icp_restatement) for block i's points against block j's cloud
  and normals under rel[i][j] (rounded to fp32 where the pair rule rounds its pose);
  assembly, pairs in ascending (i, j):  A', b' from S_ij;  M = Ad(G_j^-1) = [[R_j^T, 0], [-R_j^T [t_j]x, R_j^T]] on (omega, v);  A = M^T A' M,
  b = M^T b';  H_ii += A, H_jj += A, H_ij -= A, H_ji -= A;  g_i += b, g_j -= b;  block 0's rows and columns are dropped;
  status 2 when the total count is below n = 6 (K - 1);  Cholesky with the pair solve's pivot rule (status 3);  xi = -H^-1 g;  for b >= 1:
  R_b <- exp(omega_b) R_b, t_b <- exp(omega_b) t_b + v_b;  status 1 when max |omega_b| < tol_rot and max |v_b| < tol_trans.
`variant` plants an error in the assembly (tests): "sign" (the H_ij blocks added), "adjoint" (Ad(G_j) for Ad(G_j^-1)), "lower_left" (the
lower-left adjoint block dropped), "swapped" (a pair's two directions exchanged: S_ij assembled as if it were S_ji)."""
import math

import numpy as np

import icp_restatement as IR


def poses12_of(G):
    """[K,4,4] or [K,3,4] -> [K,12]."""
    G = np.asarray(G, dtype=np.float64)
    return np.concatenate([G[:, :3, :3].reshape(len(G), 9), G[:, :3, 3]], axis=1)


def poses44_of(G12):
    G12 = np.asarray(G12, dtype=np.float64)
    out = np.tile(np.eye(4), (len(G12), 1, 1))
    out[:, :3, :3] = G12[:, :9].reshape(-1, 3, 3)
    out[:, :3, 3] = G12[:, 9:]
    return out


def rel_poses(G12):
    """rel [K,K,12] (the diagonal included), in the kernel's operation order."""
    G12 = np.asarray(G12, dtype=np.float64)
    K = len(G12)
    rel = np.zeros((K, K, 12))
    for i in range(K):
        for j in range(K):
            Gi, Gj = G12[i], G12[j]
            for a in range(3):
                for b in range(3):
                    rel[i, j, 3 * a + b] = (Gj[a] * Gi[b] + Gj[3 + a] * Gi[3 + b]) + Gj[6 + a] * Gi[6 + b]
                rel[i, j, 9 + a] = (Gj[a] * (Gi[9] - Gj[9]) + Gj[3 + a] * (Gi[10] - Gj[10])) + Gj[6 + a] * (Gi[11] - Gj[11])
    return rel


def enabled_pairs(K, pair_mask=None):
    m = None if pair_mask is None else np.asarray(pair_mask)
    return [(i, j) for i in range(K) for j in range(K) if i != j and (m is None or m[i, j])]


def pair_correspondences(points, normals, cell_ids, rel, max_dist, pair_mask=None):
    """{(i, j): corr int [N_i]} by the pair rule's brute-force search."""
    return {(i, j): IR.correspondences(points[i], points[j], normals[j], cell_ids[j], rel[i, j], max_dist)[0] for i, j in enabled_pairs(len(points), pair_mask)}


def residuals_fp64(src, tgt, nrm, corr, pose12):
    """IR.residuals without the fp32 rounding of the pose (the derivative tests: a 1e-6 step is below the fp32 pose resolution)."""
    keep = corr >= 0
    pose12 = np.asarray(pose12, dtype=np.float64)
    q = (np.asarray(src, dtype=np.float64) @ pose12[:9].reshape(3, 3).T + pose12[9:])[keep]
    pt = np.asarray(tgt, dtype=np.float64)[corr[keep]]
    n = np.asarray(nrm, dtype=np.float64)[corr[keep]]
    r = q - pt
    e = (n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]
    return e, np.concatenate([np.cross(q, n), n], axis=1), (r * r).sum(axis=1)


def sums_fp64(src, tgt, nrm, corr, pose12):
    e, J, d2 = residuals_fp64(src, tgt, nrm, corr, pose12)
    out = [math.fsum(J[:, a] * J[:, b]) for a in range(6) for b in range(a, 6)] + [math.fsum(J[:, a] * e) for a in range(6)]
    return np.array(out + [math.fsum(e * e), math.fsum(d2), float(len(e))])


def pair_sums(points, normals, corrs, rel, round_pose=True):
    """S [K,K,30] for given correspondences ({(i, j): corr}); pairs not in corrs stay zero."""
    K = len(points)
    S = np.zeros((K, K, IR.NSUM))
    f = IR.sums_given if round_pose else sums_fp64
    for (i, j), corr in corrs.items():
        S[i, j] = f(points[i], points[j], normals[j], corr, rel[i, j])
    return S


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def adjoint_inv(G12_j, variant=None):
    """M = Ad(G_j^-1) on (omega, v)."""
    R, t = np.asarray(G12_j[:9], dtype=np.float64).reshape(3, 3), np.asarray(G12_j[9:], dtype=np.float64)
    M = np.zeros((6, 6))
    if variant == "adjoint":                                   # Ad(G_j) = [[R, 0], [[t]x R, R]]
        M[:3, :3], M[3:, 3:], M[3:, :3] = R, R, skew(t) @ R
        return M
    M[:3, :3], M[3:, 3:] = R.T, R.T
    if variant != "lower_left":
        M[3:, :3] = -R.T @ skew(t)
    return M


def unpack(s):
    """A' [6,6] and b' [6] of one pair's 30 sums, as the pair solve reads them."""
    A1 = np.zeros((6, 6))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A1[r, c] = A1[c, r] = s[k]
            k += 1
    return A1, np.asarray(s[21:27], dtype=np.float64)


def assemble(S, G12, pairs, variant=None):
    """H [6K,6K], g [6K] and the totals (count, sum e^2, sum d^2), pairs in the given (ascending) order."""
    K = len(G12)
    H, g = np.zeros((6 * K, 6 * K)), np.zeros(6 * K)
    tot = np.zeros(3)
    for i, j in pairs:
        s = S[i, j]
        A1, b1 = unpack(s)
        tot += [s[29], s[27], s[28]]
        if variant == "swapped":
            i, j = j, i
        M = adjoint_inv(G12[j], variant)
        A, b = M.T @ A1 @ M, M.T @ b1
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        H[si, si] += A
        H[sj, sj] += A
        if variant == "sign":
            H[si, sj] += A
            H[sj, si] += A
        else:
            H[si, sj] -= A
            H[sj, si] -= A
        g[si] += b
        g[sj] -= b
    return H, g, tot


def solve(H, g, tot, G12, tol_rot=1e-7, tol_trans=1e-7, eps_cond=1e-6):
    """One solve on the reduced system: (new G12, stats row, xi [6 (K - 1)]).  Status 2 / 3 return G12 itself and xi = 0."""
    G12 = np.asarray(G12, dtype=np.float64)
    K = len(G12)
    n = 6 * (K - 1)
    A, b = H[6:, 6:], g[6:]
    status, ratio, nw, nv = 0, 0.0, 0.0, 0.0
    Lc = np.zeros((n, n))
    xi = np.zeros(n)
    if tot[0] < n:
        status = 2
    else:
        ratio = math.inf
        for c in range(n):
            d = A[c, c]
            for j in range(c):
                d -= Lc[c, j] * Lc[c, j]
            rt = d / A[c, c] if A[c, c] > 0 else 0.0
            ratio = min(ratio, rt)
            if not (A[c, c] > 0) or not (d > eps_cond * A[c, c]):
                status = 3
                break
            Lc[c, c] = math.sqrt(d)
            for i in range(c + 1, n):
                v = A[i, c]
                for j in range(c):
                    v -= Lc[i, j] * Lc[c, j]
                Lc[i, c] = v / Lc[c, c]
    new = G12
    if status == 0:
        y = np.zeros(n)
        for i in range(n):
            v = -b[i]
            for j in range(i):
                v -= Lc[i, j] * y[j]
            y[i] = v / Lc[i, i]
        for i in range(n - 1, -1, -1):
            v = y[i]
            for j in range(i + 1, n):
                v -= Lc[j, i] * xi[j]
            xi[i] = v / Lc[i, i]
        new = G12.copy()
        for blk in range(1, K):
            x = xi[6 * (blk - 1):6 * blk]
            nw = max(nw, math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]))
            nv = max(nv, math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]))
            new[blk] = perturbed(G12[blk], x)
        if nw < tol_rot and nv < tol_trans:
            status = 1
    return new, np.array([tot[0], tot[1], tot[2], nw, nv, ratio, float(status)]), xi


def perturbed(G12_b, x):
    """exp(xi) G_b as the update forms it: R <- exp(omega) R, t <- exp(omega) t + v."""
    E = IR.exp_so3(x[:3])
    R, t = np.asarray(G12_b[:9]).reshape(3, 3), np.asarray(G12_b[9:])
    return np.concatenate([(E @ R).reshape(9), E @ t + np.asarray(x[3:])])


def cell_ids(points, cell):
    return [IR.grid_of(p, cell)[3] for p in points]


def refine(points, normals, G12, max_dist, iters, cell=None, pair_mask=None, tol_rot=1e-7, tol_trans=1e-7, eps_cond=1e-6, round_pose=True):
    """The whole run: (G12 [K,12], stats [iters,7]); rows after a freeze repeat the freezing row."""
    G12 = np.asarray(G12, dtype=np.float64).copy()
    K = len(points)
    cids = cell_ids(points, max_dist if cell is None else cell)
    pairs = enabled_pairs(K, pair_mask)
    rows = []
    for _ in range(iters):
        if rows and rows[-1][6] != 0:
            rows.append(rows[-1].copy())
            continue
        rel = rel_poses(G12)
        corrs = pair_correspondences(points, normals, cids, rel, max_dist, pair_mask)
        S = pair_sums(points, normals, corrs, rel, round_pose)
        H, g, tot = assemble(S, G12, pairs)
        G12, row, _ = solve(H, g, tot, G12, tol_rot, tol_trans, eps_cond)
        rows.append(row)
    return G12, np.array(rows).reshape(iters, 7)


def cost(points, normals, corrs, G12):
    """Sum of e^2 over all pairs at fixed correspondences, the poses not rounded."""
    rel = rel_poses(G12)
    return math.fsum(float((residuals_fp64(points[i], points[j], normals[j], c, rel[i, j])[0] ** 2).sum()) for (i, j), c in corrs.items())
