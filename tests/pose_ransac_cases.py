"""Seeded cases of the robust pose tests (tests/test_pose_ransac_host.py on the CPU, tests/test_hip_pose_ransac.py on the device): the two-mode
case on the ICP test solid, the exact lattice case whose counts are fixed by construction, random clouds with random triplets, and the counted
rounding bound of the fp32 triad."""
import numpy as np

import icp_cases as IC
import icp_restatement as IR

U = 2.0 ** -24
KABSCH_ATOL = 1e-5           # the tolerance tests/test_hip_pointset_ops.py::test_small_ops_vs_golden holds the weighted Kabsch kernel's pose entries to


# ------------------------------------------------------------------------------------------------------------------ the two-mode case
TWO_MODE_THRESH = 0.02
TWO_MODE_R1 = IC.rotation((0.3, -0.5, 0.8), 25.0)
TWO_MODE_T1 = np.array([0.10, -0.05, 0.08])
# host bounds of the issue (fp64 restatement, three refits): noise sigma -> (RRE in degrees, RTE)
TWO_MODE_BOUNDS = {0.0: (1e-4, 1e-7), 0.005: (0.1, 2e-3)}


def two_mode_case(minority, sigma, seed, res=32):
    """The 32^3 test solid (1,492 points) as a; a share 1 - minority of the matches follows (R1, t1) = a 25 degree motion, the rest the same motion
    composed with a further 40 degree turn about z (of the source frame: the two motions agree on that axis only, and no point of the solid is
    within thresh / (2 sin 20 deg) = 0.029 of it: the nearest cell centres are 0.044 away); Gaussian noise sigma on b.  Returns (a, b fp32, R1, t1, majority mask)."""
    pts, _ = IC.test_solid(res)
    rng = np.random.default_rng(100 + seed)
    n = len(pts)
    Rz = IC.rotation((0.0, 0.0, 1.0), 40.0)
    R2, t2 = TWO_MODE_R1 @ Rz, TWO_MODE_T1                   # the turn comes first, about the source frame's z axis
    minor = np.zeros(n, dtype=bool)
    minor[rng.permutation(n)[:int(round(minority * n))]] = True
    p = pts.astype(np.float64)
    b = np.where(minor[:, None], p @ R2.T + t2, p @ TWO_MODE_R1.T + TWO_MODE_T1)
    if sigma > 0:
        b = b + rng.normal(scale=sigma, size=b.shape)
    return pts, b.astype(np.float32), TWO_MODE_R1, TWO_MODE_T1, ~minor


def draw_triplets(n, hyps, seed):
    return np.random.default_rng(7000 + seed).integers(0, n, size=(hyps, 3)).astype(np.int32)


def pose_errors(pose12, R, t):
    p = np.asarray(pose12, dtype=np.float64)
    return IR.rre_deg(p[:9].reshape(3, 3), R), IR.rte(p[9:], t)


# ------------------------------------------------------------------------------------------------------------------ exact lattice case
EXACT_N = (3, 63, 64, 65, 1492, 3000)
EXACT_H = (1, 63, 64, 65, 4096)
EXACT_THRESH = 2.0 ** -4
EXACT_R1, EXACT_T1 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([2.0 ** -4, -3 * 2.0 ** -5, 2.0 ** -3])
EXACT_R2, EXACT_T2 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]), np.array([-2.0 ** -3, 2.0 ** -5, 2.0 ** -4])
CLEAN1, AT_THRESH, BEYOND, MOTION2, JUNK = 0, 1, 2, 3, 4


def exact_points(n, seed=0):
    """Points on the lattice of multiples of 2^-5 in [-1,1]^3.  Classes: CLEAN1 b = R1 a + t1 (a 90 degree turn about z, dyadic translation);
    AT_THRESH the same plus exactly thresh along x; BEYOND the same plus thresh (1 + 2^-23), one ulp beyond (both with a_y = t1_x, so that
    (R1 a + t1)_x = 0 and the offset is b_x itself: the residual is exact); MOTION2 b = R2 a + t2 (90 degrees about x); JUNK b a random lattice point.
    Indices 0, 1, 2 are an axis-aligned corner of CLEAN1 (legs 1/2 along x and 1/4 along y); from n >= 7 index 3 continues the first leg (0, 1, 3 are
    collinear) and 4, 5, 6 are an axis-aligned corner of MOTION2.  Under an exact pose of either motion q = R a + t is on the lattice and every
    product and sum of d^2 is exact, or (a residual against one of the two off-lattice b_x) far from thresh^2.  Returns (a, b fp32, cls)."""
    rng = np.random.default_rng(500 + 10 * n + seed)
    ai = rng.integers(-32, 33, size=(n, 3))
    cls = rng.choice([CLEAN1, AT_THRESH, BEYOND, MOTION2, JUNK], size=n, p=[0.45, 0.08, 0.08, 0.25, 0.14])
    ai[0], ai[1], ai[2] = (-8, 4, 12), (8, 4, 12), (-8, 12, 12)
    cls[:3] = CLEAN1
    if n >= 7:
        ai[3] = (24, 4, 12)
        ai[4], ai[5], ai[6] = (10, -20, -6), (10, -4, -6), (10, -20, 2)
        cls[3], cls[4:7] = CLEAN1, MOTION2
    off = (cls == AT_THRESH) | (cls == BEYOND)
    ai[off, 1] = 2                                            # a_y = t1_x = 2^-4
    a = ai / 32.0
    b = a @ EXACT_R1.T + EXACT_T1
    m2 = cls == MOTION2
    b[m2] = a[m2] @ EXACT_R2.T + EXACT_T2
    b[cls == JUNK] = rng.integers(-32, 33, size=(int((cls == JUNK).sum()), 3)) / 32.0
    b = b.astype(np.float32)
    assert np.all(b[off, 0] == 0.0)
    b[cls == AT_THRESH, 0] = np.float32(EXACT_THRESH)
    b[cls == BEYOND, 0] = np.nextafter(np.float32(EXACT_THRESH), np.float32(1.0))
    return a.astype(np.float32), b, cls


def exact_triplets(n, hyps, seed=0, all_invalid=False):
    """Triplets whose first leg and normal are axis-aligned in a and in b (R and t come out exactly), from both corners, with invalid rows: every
    h with h % 63 == 62 (over 64 waves that is every lane position once), a random tenth of the others, kinds in rotation (repeated index in each
    pair of positions, an index of -1, an index of N, the collinear triplet).  The pools are small, so equal triplets at several indices (ties)
    are the rule; the last row repeats the first valid one on purpose."""
    rng = np.random.default_rng(900 + 10 * n + hyps + seed)
    pool1 = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (2, 0, 1)] + ([(1, 3, 2), (3, 1, 2)] if n >= 7 else [])
    pool2 = [(4, 5, 6), (4, 6, 5), (5, 4, 6)] if n >= 7 else pool1
    bad = [(0, 0, 1), (0, 1, 1), (2, 1, 2), (-1, 1, 2), (0, n, 2), (1, 1, 1)] + ([(0, 1, 3), (3, 0, 1)] if n >= 7 else [])
    trip = np.zeros((hyps, 3), dtype=np.int32)
    kind = rng.choice(3, size=hyps, p=[0.3, 0.6, 0.1])        # the second motion's corner is drawn more often, the first motion has more inliers
    kind[0] = kind[0] % 2                                     # the first row is valid (H = 1 is a case)
    for h in range(hyps):
        if all_invalid or h % 63 == 62 or kind[h] == 2:
            trip[h] = bad[h % len(bad)]
        else:
            pool = pool1 if kind[h] == 0 else pool2
            trip[h] = pool[int(rng.integers(len(pool)))]
    if hyps > 1 and not all_invalid:
        valid = [h for h in range(hyps) if tuple(trip[h]) in pool1 + pool2]
        last = hyps - 1 if (hyps - 1) % 63 != 62 else hyps - 2
        if valid and last > valid[0]:
            trip[last] = trip[valid[0]]
    return trip


# ------------------------------------------------------------------------------------------------------------------ random clouds
RANDOM_SEEDS = (1, 2)
RANDOM_THRESH = 0.03


def random_case(seed, n=3000, hyps=4096):
    """A uniform cloud in [-1,1]^3 under a random pose, noise 0.01 on b, a fifth of the matches replaced by random points; random triplets (a few
    with repeated or out-of-range indices).  Returns (a, b, triplets)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    R = IC.rotation(rng.normal(size=3), rng.uniform(5, 170))
    t = rng.uniform(-0.5, 0.5, 3)
    b = a.astype(np.float64) @ R.T + t + rng.normal(scale=0.01, size=(n, 3))
    out = rng.integers(0, 5, n) == 0
    b[out] = rng.uniform(-1.5, 1.5, (int(out.sum()), 3))
    trip = rng.integers(0, n, size=(hyps, 3)).astype(np.int32)
    trip[5] = (7, 7, 9)
    trip[70] = (1, 2, n)
    trip[200] = (-3, 2, 4)
    return a, b.astype(np.float32), trip


def triad_bound(a, b, triplets):
    """Counted rounding bound of the fp32 triad against the fp64 one, per hypothesis: (well [H], bound on |dR_rc| [H], bound on |dt_r| [H]).

    With u = 2^-24 and inputs exact in fp32: a leg e = p_j - p_i carries u per component.  |e|^2 (three squares 3u each, two sums) 5u, its root
    3.5u, u1 = e1 / |e1| 5.5u.  n = e1 x e2: each product 3u, the difference u: |dn| <= (3 sqrt(2) |e1| |e2| + |n|) u = rho |n| with
    rho = (3 sqrt(2) / sin + 1) u, sin the sine of the angle between the legs.  u3 = n / |n|: 2 rho + 3.5u (|n|^2 2 rho + 3u, root rho + 2.5u,
    quotient u).  u2 = u3 x u1: 2 rho + 3.5u + 5.5u + (sqrt(2) + 1) u < 2 rho + 11.5u.  The three of a sum to 4 rho_a + 20.5u, those of b alike.
    R_rc = (v1_r u1_c + v2_r u2_c) + v3_r u3_c: the operands' errors add (unit vectors), three products and two sums of terms with
    sum_k |v_k,r| |u_k,c| <= 1 add 5u:  |dR_rc| <= (4 (rho_a + rho_b) / u + 46) u = c_R u,  c_R = 54 + 12 sqrt(2) (1 / sin_a + 1 / sin_b) <= 394 for
    sines >= 0.1 (12 sqrt(2) < 17).  t_r = b_i,r - ((R_r0 a_x + R_r1 a_y) + R_r2 a_z): |dt_r| <= (c_R |a_i|_1 + 4 |a_i|_2 + max|t|) u.  The factor 1.01
    covers the second-order terms.  well: all indices valid and distinct, both legs >= 0.1 and both sines >= 0.1, in a and in b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    trip = np.asarray(triplets, dtype=np.int64)
    n = len(a)
    i, j, k = trip[:, 0], trip[:, 1], trip[:, 2]
    ok = (trip >= 0).all(axis=1) & (trip < n).all(axis=1) & (i != j) & (i != k) & (j != k)
    ic, jc, kc = np.where(ok, i, 0), np.where(ok, j, 1 % max(n, 1)), np.where(ok, k, 2 % max(n, 1))

    def sines(p):
        e1, e2 = p[jc] - p[ic], p[kc] - p[ic]
        l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.linalg.norm(np.cross(e1, e2), axis=1) / (l1 * l2)
        return np.nan_to_num(s), np.minimum(l1, l2)

    sa, la = sines(a)
    sb, lb = sines(b)
    well = ok & (sa >= 0.1) & (sb >= 0.1) & (la >= 0.1) & (lb >= 0.1)
    with np.errstate(divide="ignore"):
        c_r = 54.0 + 12.0 * np.sqrt(2.0) * (1.0 / np.maximum(sa, 1e-30) + 1.0 / np.maximum(sb, 1e-30))
    ai = np.abs(a[ic])
    tmax = np.abs(b[ic]).max(axis=1) + ai.sum(axis=1)         # |t_r| <= |b_i,r| + |a_i|_1
    return well, 1.01 * c_r * U, 1.01 * U * (c_r * ai.sum(axis=1) + 4.0 * np.linalg.norm(ai, axis=1) + tmax)
