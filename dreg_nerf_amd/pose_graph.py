"""Pose synchronisation: the pairwise poses between the K blocks of a scene -> one pose per block (host, numpy fp64, no kernel).

An edge (i, j, P_ij, w) says x_j = R_ij x_i + t_ij (data["pose"] with src = i, tgt = j) with weight w > 0.  The result G [K,4,4] maps every
block's frame to the anchor's: G_anchor = I, and on consistent edges G_i = G_j P_ij.

Rotations   the symmetric 3K x 3K matrix M with block (j,i) += w R_ij, block (i,j) += w R_ij^T and w I on both diagonal blocks; with consistent
            edges the stacked rotations [R_1^T; ...; R_K^T]-style solution spans its three leading eigenvectors (spectral synchronisation).
            The gauge is fixed by the anchor's block and every block is projected onto SO(3) by SVD with the determinant fix.
Translations  the weighted linear least squares sum w |t_i - t_j - R_j t_ij|^2 with t_anchor = 0.
Residual    per edge, of E = G_j^-1 G_i P_ij^-1: the rotation angle in degrees (from the skew part, so small angles keep their digits) and |t|.
Robust      `iters` rounds of re-solving with w <- w0 / (1 + (theta / c_rot)^2 + (|t| / c_trans)^2): an edge that contradicts the cycles it sits
            in loses its weight.  Needs redundancy (K >= 3 with more edges than a spanning tree)."""
import numpy as np


def _pose44(P):
    P = np.asarray(P.detach().cpu().numpy() if hasattr(P, "detach") else P, dtype=np.float64).reshape(-1, 4)
    if P.shape[0] == 3:
        P = np.concatenate([P, np.array([[0.0, 0.0, 0.0, 1.0]])])
    if P.shape != (4, 4):
        raise ValueError(f"an edge's pose must be [3,4] or [4,4], got {P.shape}")
    return P


def _so3(M):
    """The rotation nearest to M (Frobenius): U diag(1, 1, det(U V^T)) V^T."""
    U, _, Vt = np.linalg.svd(M)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    return U @ D @ Vt


def rotation_angle_deg(Rm):
    """The angle of a rotation matrix in degrees: atan2(|skew part|, (trace - 1) / 2), accurate near 0 where acos of the trace is not."""
    s = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    return float(np.degrees(np.arctan2(np.linalg.norm(s), 0.5 * (np.trace(Rm) - 1.0))))


def _inv(P):
    Q = np.eye(4)
    Q[:3, :3] = P[:3, :3].T
    Q[:3, 3] = -P[:3, :3].T @ P[:3, 3]
    return Q


def _solve(K, idx, poses, w, anchor):
    M = np.zeros((3 * K, 3 * K))
    for (i, j), P, wk in zip(idx, poses, w):
        Rij = P[:3, :3]
        M[3 * j:3 * j + 3, 3 * i:3 * i + 3] += wk * Rij
        M[3 * i:3 * i + 3, 3 * j:3 * j + 3] += wk * Rij.T
        M[3 * i:3 * i + 3, 3 * i:3 * i + 3] += wk * np.eye(3)
        M[3 * j:3 * j + 3, 3 * j:3 * j + 3] += wk * np.eye(3)
    # consistent edges: R_ij = R_j^T R_i with R_i the rotation of G_i, so blockdiag(R_i) M blockdiag(R_i^T) = (D + A) (x) I_3 with the weighted
    # adjacency A and degrees D of the graph.  D + A is non-negative and, on a connected graph, irreducible: its largest eigenvalue is simple
    # with a positive eigenvector u (Perron-Frobenius), so the three leading eigenvectors of M are V with block i = u_i R_i^T Q for one
    # orthogonal Q (a reflection as often as not).
    _, vecs = np.linalg.eigh(M)
    V = vecs[:, -3:]
    Va = V[3 * anchor:3 * anchor + 3]
    R = []
    for i in range(K):
        # V_i V_a^T = u_i u_a R_i^T R_a: Q cancels, R_a = I is the gauge, and the projection removes the positive scale
        R.append(_so3((V[3 * i:3 * i + 3] @ Va.T).T))
    R[anchor] = np.eye(3)
    # translations: t_i - t_j = R_j t_ij, t_anchor = 0
    free = [i for i in range(K) if i != anchor]
    col = {b: 3 * k for k, b in enumerate(free)}
    A = np.zeros((3 * len(idx), 3 * len(free)))
    rhs = np.zeros(3 * len(idx))
    for e, ((i, j), P, wk) in enumerate(zip(idx, poses, w)):
        s = np.sqrt(wk)
        if i != anchor:
            A[3 * e:3 * e + 3, col[i]:col[i] + 3] += s * np.eye(3)
        if j != anchor:
            A[3 * e:3 * e + 3, col[j]:col[j] + 3] -= s * np.eye(3)
        rhs[3 * e:3 * e + 3] = s * (R[j] @ P[:3, 3])
    G = np.tile(np.eye(4), (K, 1, 1))
    if free:
        t = np.linalg.lstsq(A, rhs, rcond=None)[0]
        for b in free:
            G[b, :3, 3] = t[col[b]:col[b] + 3]
    for i in range(K):
        G[i, :3, :3] = R[i]
    G[anchor] = np.eye(4)
    return G


def _residuals(G, idx, poses):
    rot, trans = [], []
    for (i, j), P in zip(idx, poses):
        E = _inv(G[j]) @ G[i] @ _inv(P)
        rot.append(rotation_angle_deg(E[:3, :3]))
        trans.append(float(np.linalg.norm(E[:3, 3])))
    return np.array(rot), np.array(trans)


def synchronize(n_blocks, edges, anchor=0, robust=False, c_rot_deg=2.0, c_trans=0.05, iters=10):
    """(G [K,4,4] fp64, info) from edges (i, j, P_ij, w); info: residual_rot_deg, residual_trans, weights per edge, in the caller's order.
    robust: `iters` rounds of reweighting by the residuals with the scales c_rot_deg / c_trans (neither tuned: 2 degrees, and 0.05 = the
    project's voxel cell / ICP gate).  Raises ValueError for K < 1, an index out of range, a non-positive weight or a disconnected graph."""
    K = int(n_blocks)
    if K < 1:
        raise ValueError(f"synchronize: n_blocks = {n_blocks} (at least one block)")
    if not 0 <= int(anchor) < K:
        raise ValueError(f"synchronize: anchor {anchor} out of range for {K} blocks")
    anchor = int(anchor)
    idx, poses, w0 = [], [], []
    for i, j, P, w in edges:
        i, j = int(i), int(j)
        if not (0 <= i < K and 0 <= j < K) or i == j:
            raise ValueError(f"synchronize: edge ({i}, {j}) is not between two of {K} blocks")
        if not float(w) > 0.0:
            raise ValueError(f"synchronize: edge ({i}, {j}) has weight {w} (must be > 0)")
        idx.append((i, j)); poses.append(_pose44(P)); w0.append(float(w))
    # connected: every block is reached from the anchor
    seen, todo = {anchor}, [anchor]
    while todo:
        a = todo.pop()
        for i, j in idx:
            for u, v in ((i, j), (j, i)):
                if u == a and v not in seen:
                    seen.add(v); todo.append(v)
    if len(seen) != K:
        raise ValueError(f"synchronize: the edges do not connect blocks {sorted(set(range(K)) - seen)} to the anchor {anchor}")
    w0 = np.array(w0)
    w = w0.copy()
    G = _solve(K, idx, poses, w, anchor)
    if robust:
        for _ in range(int(iters)):
            rot, trans = _residuals(G, idx, poses)
            w = w0 / (1.0 + (rot / c_rot_deg) ** 2 + (trans / c_trans) ** 2)
            G = _solve(K, idx, poses, w, anchor)
    rot, trans = _residuals(G, idx, poses)
    return G, dict(residual_rot_deg=rot, residual_trans=trans, weights=w)
