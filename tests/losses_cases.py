"""The case table of the loss-node tests (tests/test_losses_host.py on the CPU, tests/test_hip_losses_fp64.py on the device).  Everything is generated
from the seeds and the small integer tables below.

Two families.  LATTICE: coordinates k/64, poses signed permutations (one non-orthonormal integer matrix for the point losses) with translations k/64,
radii 12/64 and 24/64, features k/16, W = k/8 times a power of two: every transformed point, difference, squared distance, logit and error sum is exact
in fp32 in any order, so the discrete decisions agree with fp64 even at equality.  GENERIC: random fp32 inputs in the distributions of
tests/test_hip_fused_losses.py::_case, admissible only where every decision clears twice the fp32 error of its distance."""
import functools

import numpy as np

E_ = 256
R_P, R_N = 12.0 / 64.0, 24.0 / 64.0          # lattice radii
GEN_R_P, GEN_R_N = 0.2, 0.4                   # generic radii (InfoNCELoss's defaults)
W_SCALE = 8.0                                 # power of two on W = k/8: logits spread over about +-12

# offsets (in 1/64) of a transformed source point from its chosen target
AT_RP = [(12, 0, 0), (0, -12, 0), (8, 8, 4), (-4, 8, -8)]                 # distance exactly r_p
IN_RP = [(11, 0, 0), (8, 8, 3), (0, 0, -11)]                              # one lattice step inside
OUT_RP = [(13, 0, 0), (8, 8, 5), (0, -13, 0)]                             # one step outside
AT_RN = [(24, 0, 0), (16, 16, 8), (0, 0, -24), (-8, 16, -16)]             # distance exactly r_n
NEAR_RN = [(23, 0, 0), (25, 0, 0), (16, 16, 7), (16, 16, 9)]
ZERO = [(0, 0, 0)]
CLOSE = [(1, 0, 0), (0, -1, 0), (4, 0, 0), (0, 4, 4)]
FAR = [(30, 30, 30), (-30, 30, -30), (30, -30, -30)]
MENUS = {"mixed": ZERO + AT_RP + IN_RP + OUT_RP + AT_RN + NEAR_RN + CLOSE + FAR, "all": ZERO + IN_RP + CLOSE, "none": FAR + OUT_RP + AT_RP}

# signed permutations of determinant +1
PERMS = [np.array(m, dtype=np.float64) for m in (
    [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]],
    [[-1, 0, 0], [0, 0, 1], [0, 1, 0]], [[0, 1, 0], [0, 0, -1], [-1, 0, 0]], [[0, 0, -1], [0, -1, 0], [-1, 0, 0]])]
SHEAR = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 2]], dtype=np.float64)      # not orthonormal, not symmetric: R^T is neither its inverse nor itself

# name -> description.  pairs: (ns, nt, positives mode, ties); ties = [(j, j')] duplicated target points, the first rows of the pair sit next to them.
# gt_mode per side (src, tgt): "rand", "zero" (all layers 0), "last0" (last layer 0, earlier layers not).  min_edges: what the host test demands of the case.
LATTICE = {
    # one workgroup of four waves holds rows of three pairs (source counts 1, 2, 1); nt = 1 / a wave edge on both sides / the unroll tail / 257, 320; total_src % 4 = 3
    "lat-shapes": dict(seed=11, L=6, pairs=[(1, 1, "all", []), (2, 63, "none", []), (1, 64, "all", []), (3, 65, "all", []), (9, 257, "one", []),
                                           (67, 320, "mixed", [(5, 69), (101, 102), (104, 105), (146, 162), (194, 210), (232, 264), (8, 40)])],
                       min_edges=dict(at_rp=1, at_rn=4, ties=7, zero_count=1, all_pos=3, one_pos=2)),
    # the staging boundary: workgroup 0 = pair 0 (2,048 targets, staged) + pair 1 (2,049, another pair's rows: global); workgroup 1 starts in pair 1
    # (not staged) and continues into pair 2 (2,048 targets it could have staged) and pair 3
    "lat-staging": dict(seed=12, L=1, pairs=[(2, 2048, "all", [(7, 71)]), (3, 2049, "mixed", [(2047, 2048)]), (2, 2048, "all", [(9, 41)]), (1, 64, "all", [])],
                        min_edges=dict(at_rp=0, at_rn=8, ties=3, zero_count=0, all_pos=3, one_pos=1)),
    # the shapes of the issue's CPU figures; every pair has positives: all five values finite
    "lat-131x70": dict(seed=13, L=6, pairs=[(131, 70, "mixed", [(3, 67), (21, 22)]), (67, 300, "mixed", [(40, 72), (18, 34)])],
                       min_edges=dict(at_rp=2, at_rn=14, ties=4, zero_count=0, all_pos=0, one_pos=0)),
    # point losses: per-side row counts 255, 256, 257, 1, 513; P = 3, L = 6; pair 0's source side zero in every layer, pair 2's source side zero in
    # the last layer only, pair 1 under the shear
    "lat-point-p3": dict(seed=14, L=6, pairs=[(255, 256, "mixed", []), (257, 1, "mixed", []), (513, 255, "mixed", [])], shear=1,
                         gt_modes=[("zero", "rand"), ("rand", "rand"), ("last0", "rand")],
                         min_edges=dict(at_rp=1, at_rn=1, ties=0, zero_count=0, all_pos=0, one_pos=0)),
    "lat-point-p1": dict(seed=15, L=1, pairs=[(1, 513, "all", [])], gt_modes=[("rand", "rand")],
                         min_edges=dict(at_rp=0, at_rn=0, ties=0, zero_count=0, all_pos=1, one_pos=1)),
}
GENERIC = {
    "gen-131x300": dict(seed=2, L=6, pairs=[(131, 300), (66, 90)]),
    "gen-5x2049": dict(seed=1, L=1, pairs=[(5, 2049), (3, 2048)]),
}
NAMES = list(LATTICE) + list(GENERIC)
INFONCE = ["lat-shapes", "lat-staging", "lat-131x70", "gen-131x300", "gen-5x2049"]
POINT = ["lat-point-p3", "lat-point-p1", "lat-131x70", "gen-131x300"]
END_TO_END = ["lat-131x70", "lat-shapes", "lat-point-p3", "gen-131x300"]


def segs_of(pairs):
    out, off = [], 0
    for pr in pairs:
        ns, nt = pr[0], pr[1]
        out.append((off, ns, off + ns, nt))
        off += ns + nt
    return out


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _labels(rng, L, n, mode):
    g = (rng.random((L, n)) > 0.4).astype(np.float64)          # different in every layer
    if n > 1:
        g[:, 0], g[:, -1] = 1.0, 0.0
        g[L - 1, 0] = 1.0
    if mode == "zero":
        g[:] = 0.0
    elif mode == "last0":
        g[L - 1] = 0.0
        if L > 1:
            g[0, 0] = 1.0
    return g


def _place(rng, tg, off, tries=300):
    """A target c and a signed permutation o of the offset such that c is a nearest target of tg[c] + o where the menu means the nearest distance
    (every offset outside CLOSE and the r_n menus); the first draw otherwise, or when no draw succeeds (the host test counts what came out)."""
    first = None
    for _ in range(tries):
        c = int(rng.integers(len(tg)))
        o = np.array(off)[rng.permutation(3)] * rng.choice([-1, 1], 3)
        if first is None:
            first = (c, tuple(int(v) for v in o))
        if tuple(off) in CLOSE + AT_RN + NEAR_RN + ZERO or ((tg - (tg[c] + o)) ** 2).sum(1).min() == (o ** 2).sum():
            return c, tuple(int(v) for v in o)
    return first


def _lattice(name):
    d = LATTICE[name]
    rng = np.random.default_rng(d["seed"])
    pairs, L = d["pairs"], d["L"]
    segs = segs_of(pairs)
    R = segs[-1][2] + segs[-1][3]
    xyz, poses = np.zeros((R, 3)), np.zeros((len(pairs), 4, 4))
    cond = rng.integers(-2, 3, (R, E_)) / 16.0
    tie_rows = []
    for p, ((ns, nt, mode, ties), (s0, _, t0, _)) in enumerate(zip(pairs, segs)):
        Rm = SHEAR if d.get("shear") == p else PERMS[(d["seed"] + p) % len(PERMS)]
        t = rng.integers(-4, 5, 3) / 64.0
        poses[p, :3, :3], poses[p, :3, 3], poses[p, 3, 3] = Rm, t, 1.0
        # distinct targets on the sub-lattice of multiples of 4 in |k| <= 28 (15^3 = 3,375 sites); the smaller sets keep to x <= 0 (1,800 sites), so that
        # a source point on the free side can have its nearest target at a chosen distance
        sites = rng.permutation(15 ** 3 if nt > 1024 else 8 * 225)[:nt]
        tg = np.stack([sites // 225, (sites // 15) % 15, sites % 15], 1) * 4 - 28
        for j, j2 in ties:
            tg[j2] = tg[j]
            cond[t0 + j2] = -cond[t0 + j]                       # the duplicate's logit is the negative: a wrong choice changes loss_row
        xyz[t0:t0 + nt] = tg / 64.0
        menu = MENUS["none" if mode == "one" else mode]
        for i in range(ns):
            if i < len(ties):                                   # next to a duplicated point: one lattice step away, every other site at least three
                c, off = ties[i][0], (1, 0, 0)
                tie_rows.append((p, i, ties[i][0], ties[i][1]))
            elif mode == "one" and i == ns - 1:
                c, off = int(rng.integers(nt)), (1, 0, 0)
            else:
                c, off = _place(rng, tg, menu[(i + p) % len(menu)])
            a = (tg[c] + np.array(off)) / 64.0
            # the source point the pose maps onto a: exact for a signed permutation (R^-1 = R^T); under the shear solve on the integers
            s = np.linalg.solve(Rm, a - t)
            xyz[s0 + i] = np.clip(np.round(s * 64.0), -64, 64) / 64.0
    gt = np.zeros((L, R))
    modes = d.get("gt_modes", [("rand", "rand")] * len(pairs))
    for (s0, ns, t0, nt), (ms, mt) in zip(segs, modes):
        gt[:, s0:s0 + ns] = _labels(rng, L, ns, ms)
        gt[:, t0:t0 + nt] = _labels(rng, L, nt, mt)
    tilde = rng.integers(-4, 9, (L, R)) / 4.0                    # |gt - tilde| from 0 to 3 in steps of 1/4: both smooth-L1 branches and |d| = 1
    # correspondences on the lattice: T x + d with d = k/64, |d| <= 2, planted zeros
    dk = rng.integers(-128, 129, (R, 3))
    dk[rng.random((R, 3)) < 0.15] = 0
    dk[rng.random((R, 3)) < 0.1] *= 0
    corr = np.zeros((R, 3))
    for p, (s0, ns, t0, nt) in enumerate(segs):
        Rm, t = poses[p, :3, :3], poses[p, :3, 3]
        corr[s0:s0 + ns] = xyz[s0:s0 + ns] @ Rm.T + t
        corr[t0:t0 + nt] = xyz[t0:t0 + nt] @ Rm + (-(Rm.T @ t))
    corr = corr + dk / 64.0
    W = rng.integers(-2, 3, (E_, E_)) / 8.0 * W_SCALE
    ov = 1.0 / (1.0 + np.exp(-rng.standard_normal(R)))
    return dict(name=name, kind="lattice", segs=segs, L=L, xyz=_f32(xyz), poses=_f32(poses), cond=_f32(cond), W=_f32(W), gt=_f32(gt), tilde=_f32(tilde),
                ov=_f32(ov), corr=_f32(corr), r_p=R_P, r_n=R_N, tie_rows=tie_rows, min_edges=d["min_edges"], modes=[pr[2] for pr in pairs])


def _generic(name):
    """The distributions of tests/test_hip_fused_losses.py::_case, with labels that differ per layer."""
    import torch
    d = GENERIC[name]
    g = torch.Generator().manual_seed(d["seed"])
    segs, L = segs_of(d["pairs"]), d["L"]
    R = segs[-1][2] + segs[-1][3]
    xyz = (torch.rand(R, 3, generator=g) - 0.5) * 1.6
    cond = torch.randn(R, E_, generator=g) * 0.3
    corr = xyz + 0.1 * torch.randn(R, 3, generator=g)
    ov = torch.sigmoid(torch.randn(R, generator=g))
    gt = (torch.rand(L, R, generator=g) > 0.4).float()
    tilde = (torch.rand(L, R, generator=g) > 0.5).float()
    poses = []
    for _ in segs:
        q, _r = torch.linalg.qr(torch.randn(3, 3, generator=g))
        if torch.det(q) < 0:
            q[:, 0] = -q[:, 0]
        T = torch.eye(4)
        T[:3, :3] = q
        T[:3, 3] = 0.05 * torch.randn(3, generator=g)
        poses.append(T)
    W = torch.randn(E_, E_, generator=g) * 0.1
    n = lambda t: _f32(t.numpy())
    return dict(name=name, kind="generic", segs=segs, L=L, xyz=n(xyz), poses=n(torch.stack(poses)), cond=n(cond), W=n(W), gt=n(gt), tilde=n(tilde),
                ov=n(ov), corr=n(corr), r_p=GEN_R_P, r_n=GEN_R_N, tie_rows=[], min_edges={}, modes=["mixed"] * len(segs))


@functools.lru_cache(maxsize=None)
def build(name):
    """The case's arrays (fp32 numpy; treat as read-only: the tests share them)."""
    c = _lattice(name) if name in LATTICE else _generic(name)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, robust=False):
    """The restatement of the whole node on the case, computed once per (case, robust)."""
    import losses_restatement as LR
    return LR.node(build(name), robust)


# ------------------------------------------------------------------------------------------------------------------ the kernels' paths, from src_off
def workgroups(segs):
    """Per workgroup of the two InfoNCE kernels (four waves = four source rows): (first pair p0 as the kernel finds it from src_off, staged?, the pairs of
    its rows)."""
    src_off, a = [], 0
    for (_, ns, _, _) in segs:
        src_off.append(a)
        a += ns
    total = a
    out = []
    for b in range((total + 3) // 4):
        p0 = 0
        while p0 + 1 < len(segs) and src_off[p0 + 1] <= b * 4:
            p0 += 1
        ps = []
        for wv in range(b * 4, min(b * 4 + 4, total)):
            p = p0
            while p + 1 < len(segs) and src_off[p + 1] <= wv:
                p += 1
            ps.append(p)
        out.append((p0, segs[p0][3] <= 2048, ps))
    return out
