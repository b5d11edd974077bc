"""Seeded cases of the joint scene-ICP tests (tests/test_scene_icp_host.py on the CPU, tests/test_hip_scene_icp.py on the device): partial
views of the test solid under known motions, exactly representable K-block lattice scenes, random K-block scenes."""
import numpy as np

import icp_cases as IC
import icp_restatement as IR
import scene_icp_restatement as SR

# the views of the test solid (predicates on the anchor-frame coordinates) and block b's true motion (axis, degrees, direction, length);
# block 0 is the anchor.  The three-view case is the first three.
VIEW_MASKS = (lambda p: p[:, 0] < 0.2,
              lambda p: (p[:, 0] > -0.3) & (p[:, 1] < 0.45),
              lambda p: p[:, 1] > -0.15,
              lambda p: (p[:, 2] < 0.35) & (p[:, 0] > -0.45))
VIEW_MOTIONS = (None,
                ((0.3, -0.5, 0.8), 3.0, (0.5, -0.7, 0.4), 0.03),
                ((-0.6, 0.2, 0.5), 4.0, (-0.3, 0.4, 0.8), 0.036),
                ((0.7, 0.6, -0.2), 2.0, (0.6, 0.5, -0.4), 0.02))


def view_case(K=3, res=32, fp32=True, deg_len=None):
    """K partial views of IC.test_solid(res): (points [K] of [N_b,3], normals [K], G_true [K,12]); a run starts from the identity, so the initial
    error is the whole motion.  Block b's points are R_b^T (x - t_b) of the view's anchor-frame points x, its normals R_b^T n.  fp32=False keeps
    both in fp64 (the derivative tests: residuals of 1e-16 at the true poses).  deg_len = (degrees, length) replaces every motion's size (the
    benchmark's starts), the axes and directions stay."""
    pts, nrm = IC.test_solid(res)
    points, normals, G = [], [], []
    for b in range(K):
        m = VIEW_MASKS[b](pts)
        if VIEW_MOTIONS[b] is None:
            R, t = np.eye(3), np.zeros(3)
        else:
            axis, deg, d, length = VIEW_MOTIONS[b]
            if deg_len is not None:
                deg, length = deg_len
            R, t = IC.rotation(axis, deg), length * np.asarray(d) / np.linalg.norm(d)
        p = (pts[m].astype(np.float64) - t) @ R
        n = nrm[m].astype(np.float64) @ R
        points.append(p.astype(np.float32) if fp32 else p)
        normals.append(n.astype(np.float32) if fp32 else n)
        G.append(IR.pose12_of(R, t))
    return points, normals, np.array(G)


def identity_poses(K):
    return np.tile(IR.pose12_of(np.eye(3), np.zeros(3)), (K, 1))


def worst_errors(G12, G_true):
    """(worst RRE in degrees, worst RTE) over the blocks."""
    return (max(IR.rre_deg(a[:9].reshape(3, 3), b[:9].reshape(3, 3)) for a, b in zip(G12, G_true)),
            max(IR.rte(a[9:], b[9:]) for a, b in zip(G12, G_true)))


# ------------------------------------------------------------------------------------------------------------------ exact scenes
EXACT_MAX_DIST = IC.EXACT_MAX_DIST
_ROT90 = ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]])
_DYADIC = ([0.0, 0.0, 0.0], [2.0 ** -4, -3 * 2.0 ** -5, 2.0 ** -3], [-2.0 ** -3, 2.0 ** -5, 2.0 ** -4], [3 * 2.0 ** -5, 2.0 ** -4, -2.0 ** -5])


def exact_scene(sizes, seed=0):
    """len(sizes) blocks of lattice points (multiples of 2^-5 in [-1,1]^3 in the anchor frame), block b under a 90 degree rotation and a dyadic
    translation (the anchor's the identity), axis unit normals (one in 16 zero): rel, q, d^2, e, J are exact in fp32 and every sum is exact in
    fp64.  Returns (points [K], normals [K], G12 [K,12])."""
    rng = np.random.default_rng(7000 + 31 * seed + sum((k + 1) * s for k, s in enumerate(sizes)))
    points, normals, G = [], [], []
    for b, n in enumerate(sizes):
        R, t = np.array(_ROT90[b], dtype=np.float64), np.array(_DYADIC[b])
        flat = rng.choice(65 ** 3, size=n, replace=False)
        x = (np.stack([flat % 65, (flat // 65) % 65, flat // (65 * 65)], axis=1) - 32) / 32.0
        axes = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n)[:, None]
        axes[rng.integers(0, 16, n) == 0] = 0.0
        points.append(((x - t) @ R).astype(np.float32))
        normals.append((axes @ R).astype(np.float32))
        G.append(IR.pose12_of(R, t))
    return points, normals, np.array(G)


def random_scene(sizes, seed=0):
    """len(sizes) blocks of random points around one shared random cloud, each under a random pose with random unit normals (one in 20 zero), the
    poses handed to the run off the true ones: (points [K], normals [K], G12 [K,12])."""
    rng = np.random.default_rng(9000 + 17 * seed + sum((k + 1) * s for k, s in enumerate(sizes)))
    base = rng.uniform(-1, 1, (1500, 3))
    points, normals, G = [], [], []
    for b, n in enumerate(sizes):
        R = np.eye(3) if b == 0 else IC.rotation(rng.normal(size=3), rng.uniform(5, 40))
        t = np.zeros(3) if b == 0 else rng.uniform(-0.3, 0.3, 3)
        x = base[rng.integers(0, len(base), n)] + rng.normal(scale=0.03, size=(n, 3))
        nr = rng.normal(size=(n, 3))
        nr /= np.linalg.norm(nr, axis=1, keepdims=True)
        nr[rng.integers(0, 20, n) == 0] = 0.0
        points.append(((x - t) @ R).astype(np.float32))
        normals.append(nr.astype(np.float32))
        G.append(IR.pose12_of(R, t))
    return points, normals, np.array(G)


# the scenes of the per-pair bit-for-bit test: K = 2, 3, 4, sizes from {1, 255, 256, 257, 1492} mixed within a scene, so that one-workgroup and
# multi-workgroup pairs sit next to each other in the pair table; None = all pairs, else a mask with holes
SCENE_SIZES = ((257, 1492), (1, 256), (1492, 255, 257), (256, 1, 1492), (1492, 257, 1, 255), (255, 256, 1492, 257))


def holed_mask(K):
    m = np.ones((K, K), dtype=np.uint8)
    m[0, K - 1] = 0
    if K > 2:
        m[2, 1] = 0
        m[1, 0] = 0
    return m
