"""What the fused loss node (csrc/losses.hip, fused_losses._RegLossFn) computes, restated stage by stage in numpy fp64 with the buffers the kernels
produce, and next to every inexact stage a bound on the fp32 error derived from the kernel's operation count.  Formulation: train_nerf_regtr.py:186-229,
correspondence_loss.py:16-51, feature_loss.py:24-73 as dreg_nerf_amd/losses.py states them (tests/test_losses_host.py holds this file to that torch
formulation in fp64).

Row space: R rows = every pair's (src | tgt) key points; segs = [(s0, ns, t0, nt)] per pair, as attn_ops.ProblemTable.segs."""
import math

import numpy as np

from dreg_nerf_amd.losses import LOSS_WEIGHTS

EPS = 1e-6
U = 2.0 ** -24                      # unit roundoff of fp32 (half an ulp, relative)
START = float(np.float32(3.4e38))   # infonce_nn_kernel's start value: a squared distance that is not below it never wins a comparison


def f64(a):
    return np.asarray(a, dtype=np.float64)


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------ rigid maps
def side_maps(pose):
    """The two 3x4 maps of a pair: the source side applies (R, t), the target side (R^T, -R^T t) — a transpose, not an inverse."""
    pose = f64(pose)
    R, t = pose[:3, :3], pose[:3, 3]
    return np.concatenate([R, t[:, None]], 1), np.concatenate([R.T, -(R.T @ t)[:, None]], 1)


def apply_map(M, x):
    return f64(x) @ M[:, :3].T + M[:, 3]


def map_error(M, x):
    """|fp32 (x0 M0 + x1 M1 + x2 M2 + t) - exact| per component: three products and three additions, no contraction; every term passes through at most
    four roundings."""
    return gamma(4) * (np.abs(f64(x)) @ np.abs(M[:, :3]).T + np.abs(M[:, 3]))


# ------------------------------------------------------------------------------------------------------------------ point losses
def pseudo_huber(d, scale=0.5):
    return np.sqrt((d / scale) ** 2 + 1.0) - 1.0


def pseudo_huber_grad(d, scale=0.5):
    return (d / scale ** 2) / np.sqrt((d / scale) ** 2 + 1.0)


def point_losses(gt, tilde, ov, corr, xyz, poses, segs, robust, d_exact=False):
    """reg_point_losses_kernel.  gt, tilde [L,R] (tilde may be None: column 1 stays 0), ov [R], corr [R,3], xyz [R,3], poses [P,4,4].
    Returns partial [2P,4] = per (pair, side) (BCE sum, smooth-L1 sum, error sum, label sum), d_ov [R], d_corr [R,3], factor [2P] (the correspondence
    weight of the side, w_corr / P folded in), d [R,3] (corr - T x), and the fp32 error bounds bce_bound [2P], err_bound [2P], d_corr_bound [R,3].
    d_exact: the caller states that corr - T x is exact in fp32 (lattice inputs), so the bounds carry no term for it."""
    gt, ov, corr, xyz = f64(gt), f64(ov), f64(corr), f64(xyz)
    L, R = gt.shape
    P = len(segs)
    wo, wr = LOSS_WEIGHTS["overlap"], LOSS_WEIGHTS["corr"]
    partial = np.zeros((2 * P, 4))
    d_ov, d_corr, d_all = np.zeros(R), np.zeros((R, 3)), np.zeros((R, 3))
    factor, bce_bound, err_bound = np.zeros(2 * P), np.zeros(2 * P), np.zeros(2 * P)
    d_corr_bound = np.zeros((R, 3))
    for p, (s0, ns, t0, nt) in enumerate(segs):
        maps = side_maps(poses[p])
        for side, (r0, n) in enumerate(((s0, ns), (t0, nt))):
            rows = slice(r0, r0 + n)
            x, tt = gt[L - 1, rows], ov[rows]                       # BCEWithLogits(input = labels, target = prediction), LAST layer
            e = np.exp(-np.abs(x))
            l1p = np.log1p(e)
            bce_rows = np.maximum(x, 0.0) - x * tt + l1p
            # per row: the product, the subtraction and the final addition round once each (U relative); expf and log1pf are taken at 2 ulp = 4 U
            # relative each, the former passing through d log1p / d e = 1 / (1 + e)
            row_b = U * np.abs(x * tt) + U * np.abs(np.maximum(x, 0.0) - x * tt) + 4 * U * e / (1.0 + e) + 4 * U * l1p + U * np.abs(bce_rows)
            sl1 = 0.0
            if tilde is not None:
                dd = gt[:, rows] - f64(tilde)[:, rows]
                a = np.abs(dd)
                sl1 = np.where(a < 1.0, 0.5 * dd * dd, a - 0.5).sum()
            wsum = gt[:, rows].sum()                                # over ALL layers: the reference's [nl,N,1] x [N] broadcast
            M = maps[side]
            d = corr[rows] - apply_map(M, xyz[rows])
            d_all[rows] = d
            d_err = np.zeros_like(d) if d_exact else map_error(M, xyz[rows]) + U * np.abs(d)
            if robust:
                s = np.sqrt((d / 0.5) ** 2 + 1.0)
                val = np.abs(s - 1.0)
                # d / 0.5 is exact; square, + 1, sqrt and - 1 round once each (the last is exact below 2); |ph'| <= 2 carries the error of d
                val_b = U * ((d / 0.5) ** 2 + (d / 0.5) ** 2 + 1.0) / (2.0 * s) + U * s + U * val + 2.0 * d_err
                g = pseudo_huber_grad(d)
                # d / 0.25 exact; the denominator as above (2 U relative after the sqrt halves the first two), the division rounds once;
                # |d g / d d| <= 4 carries the error of d
                g_b = 3 * U * np.abs(g) + 4.0 * d_err
            else:
                val, val_b = np.abs(d), d_err
                g, g_b = np.sign(d), np.zeros_like(d)               # a sign flips only where |d| <= d_err: the caller excludes those entries
            err_rows = val.sum(1)
            err = err_rows.sum()
            ratio = wsum / max(wsum, EPS)
            f = ratio * wr / P
            b = 2 * p + side
            partial[b] = (bce_rows.sum(), sl1, err, wsum)
            factor[b] = f
            bce_bound[b] = row_b.sum() + U * abs(bce_rows.sum())
            err_bound[b] = (val_b.sum(1) + 3 * U * err_rows).sum() + U * err      # three fp32 additions per row, the fp64 block sum, one final rounding
            d_ov[rows] = -x / (ns + nt) * wo / P
            d_corr[rows] = g * f
            d_corr_bound[rows] = (g_b + 2 * U * np.abs(g)) * f                      # + the rounding of the factor (one division) and of the product
    return dict(partial=partial, d_ov=d_ov, d_corr=d_corr, factor=factor, d=d_all, bce_bound=bce_bound, err_bound=err_bound, d_corr_bound=d_corr_bound)


# ------------------------------------------------------------------------------------------------------------------ InfoNCE: decisions
def pair_distances(xyz, pose, seg):
    """Transformed source points, the [ns, nt] distance matrix of a pair, and E [ns, nt]: the worst absolute fp32 error of a distance as the kernels form
    it (map, three differences, three squares, two additions, sqrtf), from the coordinate magnitudes."""
    s0, ns, t0, nt = seg
    xyz = f64(xyz)
    M = side_maps(pose)[0]
    a = apply_map(M, xyz[s0:s0 + ns])
    q = xyz[t0:t0 + nt]
    diff = a[:, None, :] - q[None, :, :]
    dist = np.sqrt((diff ** 2).sum(-1))
    e_diff = map_error(M, xyz[s0:s0 + ns])[:, None, :] + U * np.abs(diff)              # per component
    E = np.sqrt((e_diff ** 2).sum(-1)) + 4 * U * dist                                  # squares, two sums, sqrt: at most 4 U relative on the distance
    return a, dist, E


def infonce_decisions(xyz, poses, segs, r_p, r_n):
    """infonce_nn_kernel + infonce_count_kernel and the column set of infonce_rows_kernel.  Per pair: nn [ns] (lowest index on equal squared distance;
    0 where no squared distance compares below the start value), mask [ns], count, included [ns, nt] = (j == nn) | not (dist < r_n), dist, E.
    The radii are the fp32 values the kernels receive."""
    r_p, r_n = float(np.float32(r_p)), float(np.float32(r_n))
    out = []
    for p, seg in enumerate(segs):
        a, dist, E = pair_distances(xyz, poses[p], seg)
        d2 = ((a[:, None, :] - f64(xyz)[seg[2]:seg[2] + seg[3]][None]) ** 2).sum(-1)
        with np.errstate(invalid="ignore"):
            wins = d2 < START
        d2w = np.where(wins, d2, np.inf)
        nn = np.argmin(d2w, axis=1)                                                    # first occurrence = lowest index
        none = ~wins.any(axis=1)
        nn[none] = 0
        near = np.sqrt(d2w[np.arange(len(nn)), nn])
        mask = ((near < r_p) & ~none).astype(np.float64)
        with np.errstate(invalid="ignore"):
            inc = ~(dist < r_n)
        inc[np.arange(len(nn)), nn] = True
        out.append(dict(nn=nn.astype(np.int64), mask=mask, count=float(mask.sum()), included=inc, dist=dist, d2=d2, E=E, near=near))
    return out


def decision_margins(dec, r_p, r_n):
    """Of one pair's decisions: the smallest of |near - r_p|, |dist - r_n| and (second nearest - nearest), each divided by its 2 E.  > 1: every decision is
    the same in fp32 and fp64."""
    r_p, r_n = float(np.float32(r_p)), float(np.float32(r_n))
    dist, E, nn = dec["dist"], dec["E"], dec["nn"]
    rows = np.arange(len(nn))
    m = [np.min(np.abs(dist[rows, nn] - r_p) / (2 * E[rows, nn])), np.min(np.abs(dist - r_n) / (2 * E))]
    if dist.shape[1] > 1:
        other = dist.copy()
        other[rows, nn] = np.inf
        j2 = np.argmin(other, axis=1)
        m.append(np.min((dist[rows, j2] - dist[rows, nn]) / (E[rows, j2] + E[rows, nn])))
    return m


# ------------------------------------------------------------------------------------------------------------------ InfoNCE: rows
def row_bound_factor(nt):
    """(4 (ceil(nt / 64) + 6) + 4) 2^-24: one rescale-and-add per strided step of a lane and six shuffle merges, a few ulp each on the running sum,
    then logf and the final subtraction."""
    return (4 * (math.ceil(nt / 64) + 6) + 4) * U


def infonce_rows(logits, dec, scale):
    """infonce_rows_kernel on one pair: logits [ns, nt] (fp64 view of what the kernel reads), dec one entry of infonce_decisions, scale = w_feat / P.
    Returns loss_row [ns], grad [ns, nt], lse, lnn, soft [ns, nt] (softmax over the included columns, 0 elsewhere), k [ns], and the bounds
    B [ns] (on loss_row) and grad_bound [ns, nt]."""
    lg = f64(logits)
    ns, nt = lg.shape
    nn, mask, inc, count = dec["nn"], dec["mask"], dec["included"], dec["count"]
    rows = np.arange(ns)
    masked = np.where(inc, lg, -np.inf)
    mx = masked.max(1)
    se = np.exp(masked - mx[:, None]).sum(1)
    lse = mx + np.log(se)
    lnn = lg[rows, nn]
    loss_row = mask * (lse - lnn)
    soft = np.where(inc, np.exp(lg - lse[:, None]), 0.0)
    k = np.where((mask > 0) & (count > 0), scale / max(count, 1.0), 0.0)
    onehot = np.zeros_like(lg)
    onehot[rows, nn] = 1.0
    grad = k[:, None] * (soft - onehot)
    B = row_bound_factor(nt) * np.maximum(1.0, np.maximum(np.abs(lse), np.abs(lnn)))
    # the entry the kernel forms with error is k * expf(v - lse): relative error B (from lse, the subtraction and expf); the one-hot's - 1 and the product
    # with k round within one ulp of k.  At column nn the bound is taken on that softmax term: the subtraction of the one-hot cancels, and no fp32 lse
    # could hold an error relative to the difference.
    ulp_k = 2 * U * k
    grad_bound = B[:, None] * (k[:, None] * soft) + ulp_k[:, None]
    return dict(loss_row=loss_row, grad=grad, lse=lse, lnn=lnn, soft=soft, k=k, B=B, grad_bound=grad_bound)


# ------------------------------------------------------------------------------------------------------------------ final
def final(partial, loss_rows, counts, segs, L):
    """reg_losses_final_kernel: the five means over the pairs (overlap, nerf_cont, feature, corr, total) from partial [2P,4], the per-pair loss_row arrays
    and counts; feature = sum / count per pair with 0 / 0 = nan."""
    partial = f64(partial)
    P = len(segs)
    acc = np.zeros(4)
    for p, (s0, ns, t0, nt) in enumerate(segs):
        a, b = partial[2 * p], partial[2 * p + 1]
        n = ns + nt
        acc[0] += (a[0] + b[0]) / n
        acc[1] += (a[1] + b[1]) / (n * L)
        f, c = float(f64(loss_rows[p]).sum()), float(counts[p])
        with np.errstate(invalid="ignore", divide="ignore"):
            acc[2] += np.float64(f) / np.float64(c)
        acc[3] += a[2] * (a[3] / max(a[3], EPS)) + b[2] * (b[3] / max(b[3], EPS))
    out = acc / P
    w = LOSS_WEIGHTS
    total = w["overlap"] * out[0] + w["nerf_cont"] * out[1] + w["feature"] * out[2] + w["corr"] * out[3]
    return np.concatenate([out, [total]])


def total_of(out4):
    """out[4] as the kernels form it from their own fp32 out[0..3] with fp32 weights, and its bound: one product rounding per weight that is not 1 and three
    additions, each on at most the sum of the absolute terms."""
    w = [float(np.float32(LOSS_WEIGHTS[k])) for k in ("overlap", "nerf_cont", "feature", "corr")]
    terms = [w[i] * float(out4[i]) for i in range(4)]
    return sum(terms), 4 * U * sum(abs(t) for t in terms)


# ------------------------------------------------------------------------------------------------------------------ GEMM chain
def wsym(W):
    W = f64(W)
    return np.triu(W) + np.triu(W).T


def product(A, B, eA=None, eB=None):
    """A @ B with the running fp32 bound of a length-K product in any order, K 2^-24 (|A| |B|), plus the carried bounds of inexact operands."""
    A, B = f64(A), f64(B)
    K = A.shape[1]
    C = A @ B
    e = gamma(K) * (np.abs(A) @ np.abs(B))
    if eA is not None:
        e = e + eA @ np.abs(B)
    if eB is not None:
        e = e + np.abs(A) @ eB
    if eA is not None and eB is not None:
        e = e + eA @ eB
    return C, e


def gemm_forward(cond, W, segs):
    """Levels 0 and 1: q = f_src Wsym and every pair's logits = q f_tgt^T, each with its bound."""
    cond = f64(cond)
    ws = wsym(W)
    out = []
    for (s0, ns, t0, nt) in segs:
        q, eq = product(cond[s0:s0 + ns], ws)
        lg, el = product(q, cond[t0:t0 + nt].T, eA=eq)
        out.append(dict(q=q, eq=eq, logits=lg, elogits=el))
    return ws, out


def gemm_backward(cond, ws, fwd, rows, segs):
    """Levels 2 and 3 from every pair's logits gradient G (rows[p]["grad"], bound rows[p]["grad_bound"] for exact logits): dq = G f_tgt,
    d f_tgt = G^T q, d f_src = dq Wsym.  The bound of G first takes in the error of the logits the kernel read: a perturbation delta of a row's included
    logits moves a softmax entry by at most (exp(2 delta) - 1) times the entry.  Returns d_cond [R,256] and its bound."""
    cond = f64(cond)
    d_cond, e_cond = np.zeros_like(cond), np.zeros_like(cond)
    for (s0, ns, t0, nt), f, r in zip(segs, fwd, rows):
        delta = np.where(r["soft"] > 0, f["elogits"], 0.0).max(1)
        eG = r["grad_bound"] + np.expm1(2 * delta)[:, None] * (r["k"][:, None] * r["soft"]) * (1 + r["B"][:, None])
        G = r["grad"]
        ft = cond[t0:t0 + nt]
        dq, edq = product(G, ft, eA=eG)
        dft, edft = product(G.T, f["q"], eA=eG.T, eB=f["eq"])
        dfs, edfs = product(dq, ws, eA=edq)
        d_cond[s0:s0 + ns], e_cond[s0:s0 + ns] = dfs, edfs
        d_cond[t0:t0 + nt], e_cond[t0:t0 + nt] = dft, edft
    return d_cond, e_cond


# ------------------------------------------------------------------------------------------------------------------ the whole node
def node(c, robust, tilde="given"):
    """Every stage on a case of tests/losses_cases.py (exact logits: the fp64 products).  tilde = None: the deferred form's first half."""
    segs = c["segs"]
    P, L = len(segs), c["gt"].shape[0]
    pl = point_losses(c["gt"], c["tilde"] if tilde is not None else None, c["ov"], c["corr"], c["xyz"], c["poses"], segs, robust, d_exact=c["kind"] == "lattice")
    dec = infonce_decisions(c["xyz"], c["poses"], segs, c["r_p"], c["r_n"])
    ws, fwd = gemm_forward(c["cond"], c["W"], segs)
    scale = LOSS_WEIGHTS["feature"] / P
    rows = [infonce_rows(f["logits"], d, scale) for f, d in zip(fwd, dec)]
    out = final(pl["partial"], [r["loss_row"] for r in rows], [d["count"] for d in dec], segs, L)
    d_cond, e_cond = gemm_backward(c["cond"], ws, fwd, rows, segs)
    return dict(point=pl, dec=dec, wsym=ws, fwd=fwd, rows=rows, out=out, d_cond=d_cond, e_cond=e_cond)
