"""fp64 restatement (numpy, no autograd) of the field's input gradients of csrc/field_input_grad.hip: dL/dx and dL/ddir at points
for two upstream gradients, parameters frozen, and their sums along rays.  Built on tests/field_points_restatement.py's forward record (imported,
not edited) and tests/ngp_grad_restatement.py's cells.

The rule.  Point i with forward record hd, h1, h2 (only their signs are used: the ReLU gates), raw[0] = h0, c (the fp16 colour), position x and
direction d (fp32, used as given), upstream gradients g_sigma, g_rgb:
    dL/dh0 = g_sigma exp(min(h0 - 1, 15)) inside the model aabb (strictly), 0 outside          dL/do = g_rgb c (1 - c)
    d2 = relu'(h2) W3[0:3]^T do,   d1 = relu'(h1) W2^T d2,   dsh[j] = sum_i W1[i][j] d1[i]  (j = 0..15),
    dout[0] = dh0, dout[k] = sum_i W1[i][15 + k] d1[i]  (k = 1..15),   dh = relu'(hd) W2d^T dout,   de = W1d^T dh
    dL/dd_c = sum_j dsh[j] dsh4_j/dd_c                 (SH4: the monomials below, differentiated term by term)
    du_c    = sum_l scale_l sum_corners (+-1)(w_a w_b)(de[2l] t_0 + de[2l+1] t_1)
    dL/dx_c = du_c / (hi_c - lo_c) where 0 < u_c < 1 strictly (u before the clamp), exactly 0 on a clamped axis.
u, pos, floor and w of every level are formed in fp32 exactly as the kernel forms them (they decide the cell and the clamp), everything after them
in fp64.  Every element comes with M, the same sum with every term replaced by its absolute value, and n, the terms of its last sum: the bound of
tests/test_hip_field_input_grad.py is (C + n) 2^-24 M.

Ray level (ray_sums64): for a list in canonical order with x_k = o + t_k d and dirs_k = d, t_k constant,
    dL/do[r] = sum_{k in r} dL/dx_k,     dL/dd[r] = sum_{k in r} (t_k dL/dx_k + dL/ddir_k).

`mutate` names one deliberate error (MUTATIONS); tests/test_field_input_grad_host.py shows that each lands well beyond the bound."""
import numpy as np

import ngp_grad_restatement as GR

MUTATIONS = ("corner", "sign", "w_own", "no_ext", "sh_cols", "t_next", "no_clamp")

C1, C2, C3, C4, C5 = 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.54627421529603959, 0.59004358992664352
C6, C7, C8, C9 = 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769
# SH4 of a direction (tcnn's convention, oracle.ngp_oracle.sh4) as monomials (coefficient, power of x, of y, of z)
SH4 = (((0.28209479177387814, 0, 0, 0),), ((-C1, 0, 1, 0),), ((C1, 0, 0, 1),), ((-C1, 1, 0, 0),), ((C2, 1, 1, 0),), ((-C2, 0, 1, 1),),
       ((C3, 0, 0, 2), (-0.31539156525251999, 0, 0, 0)), ((-C2, 1, 0, 1),), ((C4, 2, 0, 0), (-C4, 0, 2, 0)), ((-3 * C5, 2, 1, 0), (C5, 0, 3, 0)),
       ((C6, 1, 1, 1),), ((C7, 0, 1, 0), (-5 * C7, 0, 1, 2)), ((5 * C8, 0, 0, 3), (-3 * C8, 0, 0, 1)), ((C7, 1, 0, 0), (-5 * C7, 1, 0, 2)),
       ((C9, 2, 0, 1), (-C9, 0, 2, 1)), ((-C5, 3, 0, 0), (3 * C5, 1, 2, 0)))


def sh4_value(d):
    """SH4 [N,16] of the monomials (fp64): what tests/test_field_input_grad_host.py compares with the oracle's sh4."""
    d = np.asarray(d, np.float64)
    return np.stack([sum(k * d[:, 0] ** a * d[:, 1] ** b * d[:, 2] ** c for k, a, b, c in poly) for poly in SH4], 1)


def sh4_jacobian(d):
    """(J, Jabs, terms): J [N,16,3] = dSH4_j/dd_c at the fp32 directions, Jabs the same with every monomial's absolute value, terms [16,3] the
    monomials of each entry."""
    d = np.asarray(d, np.float32).astype(np.float64)
    n = len(d)
    J, Ja, terms = np.zeros((n, 16, 3)), np.zeros((n, 16, 3)), np.zeros((16, 3))
    for j, poly in enumerate(SH4):
        for k, *pw in poly:
            for c in range(3):
                if pw[c] == 0:
                    continue
                q = list(pw)
                q[c] -= 1
                m = k * pw[c] * d[:, 0] ** q[0] * d[:, 1] ** q[1] * d[:, 2] ** q[2]
                J[:, j, c] += m
                Ja[:, j, c] += np.abs(m)
                terms[j, c] += 1
    return J, Ja, terms


def unit_axes(x, aabb):
    """u fp32 clamped [N,3], inside [N] (all axes strictly), open [N,3] (the axis strictly inside: not clamped), as ngp_unit_cube forms them."""
    x = np.asarray(x, np.float32)
    lo, hi = np.asarray(aabb[:3], np.float32), np.asarray(aabb[3:], np.float32)
    u = ((x - lo) / (hi - lo)).astype(np.float32)
    op = (u > 0) & (u < 1)
    return np.clip(u, 0, 1).astype(np.float32), op.all(axis=1), op


def encoding_jacobian(u, table, lv, mutate=None):
    """(E, Eabs): E [N, 2L, 3] = d enc_{2l+f} / du_c at the fp32 unit coordinates u (piecewise constant in the other two weights' cell), Eabs the
    sum of the absolute corner terms.  table: the fp16 table's values, [entries, 2]."""
    nl = len(lv["scale"])
    E, Ea = np.zeros((len(u), 2 * nl, 3)), np.zeros((len(u), 2 * nl, 3))
    for l in range(nl):
        g, w = GR.level_cells(u, lv["scale"][l], np.float32)
        s = float(lv["scale"][l])
        for corner, (t, wa, sg) in enumerate(GR._corners(g, w, lv, l, table)):
            if mutate == "corner" and l == nl - 1 and corner == 7:
                continue
            for c in range(3):
                a, b = (c + 1) % 3, (c + 2) % 3
                sign = -sg[c] if (mutate == "sign" and c == 1) else sg[c]
                ww = wa[:, c] * wa[:, a] if mutate == "w_own" else wa[:, a] * wa[:, b]
                E[:, 2 * l:2 * l + 2, c] += (s * sign * ww)[:, None] * t
                Ea[:, 2 * l:2 * l + 2, c] += (s * ww)[:, None] * np.abs(t)
    return E, Ea


class Result:
    pass


def input_grad64(record, weights, table, dirs, g_sigma, g_rgb, levels, model_aabb, mutate=None):
    """record: arrays [N, .] or broadcastable [1, .]: raw (column 0 = h0), c, hd, h1, h2 (gates = value > 0), and x fp32 [N,3]; weights: the five
    matrices' fp16 values (d1, d2, c1, c2, c3); table: the fp16 table's values [entries,2]; dirs fp32 [N,3]; g_sigma [N] / g_rgb [N,3] or None.
    Returns gx, gxM [N,3], gd, gdM [N,3], nx, nd (terms of the last sums), inside [N], open [N,3], de, dsh."""
    assert mutate is None or mutate in MUTATIONS
    x = np.asarray(record["x"], np.float32)
    Np = len(x)
    gs = np.zeros(Np) if g_sigma is None else np.asarray(g_sigma, np.float64)
    gc = np.zeros((Np, 3)) if g_rgb is None else np.asarray(g_rgb, np.float64)
    u, inside, op = unit_axes(x, model_aabb)
    h0 = np.broadcast_to(np.asarray(record["raw"], np.float64), (Np, 16))[:, 0]
    c = np.broadcast_to(np.asarray(record["c"], np.float64), (Np, 3))
    ex = np.exp(np.minimum(h0 - 1.0, 15.0))
    dh0, dh0M = np.where(inside, gs * ex, 0.0), np.where(inside, np.abs(gs) * ex, 0.0)
    dO = gc * c * (1.0 - c)
    W = {k: np.asarray(v, np.float64) for k, v in weights.items()}
    gate = {k: np.broadcast_to(np.asarray(record[k], np.float64), (Np, 64)) > 0 for k in ("hd", "h1", "h2")}
    A = np.abs
    d2, d2M = (dO @ W["c3"][:3]) * gate["h2"], (A(dO) @ A(W["c3"][:3])) * gate["h2"]
    d1, d1M = (d2 @ W["c2"]) * gate["h1"], (d2M @ A(W["c2"])) * gate["h1"]
    shc = slice(16, 32) if mutate == "sh_cols" else slice(0, 16)
    dsh, dshM = d1 @ W["c1"][:, shc], d1M @ A(W["c1"][:, shc])
    dout, doutM = np.zeros((Np, 16)), np.zeros((Np, 16))
    dout[:, 0], doutM[:, 0] = dh0, dh0M
    dout[:, 1:], doutM[:, 1:] = d1 @ W["c1"][:, 16:31], d1M @ A(W["c1"][:, 16:31])
    dh, dhM = (dout @ W["d2"]) * gate["hd"], (doutM @ A(W["d2"])) * gate["hd"]
    de, deM = dh @ W["d1"], dhM @ A(W["d1"])
    out = Result()
    J, Ja, terms = sh4_jacobian(dirs)
    out.gd, out.gdM = np.einsum("nj,njc->nc", dsh, J), np.einsum("nj,njc->nc", dshM, Ja)
    out.nd = terms.sum(0)[None].repeat(Np, 0)
    E, Ea = encoding_jacobian(u, np.asarray(table).reshape(-1, 2), levels, mutate)
    ext = np.asarray(model_aabb[3:], np.float32).astype(np.float64) - np.asarray(model_aabb[:3], np.float32).astype(np.float64)
    if mutate == "no_ext":
        ext = np.ones(3)
    keep = np.ones_like(op) if mutate == "no_clamp" else op
    out.gx, out.gxM = np.einsum("nk,nkc->nc", de, E) / ext * keep, np.einsum("nk,nkc->nc", deM, Ea) / ext * keep
    out.nx = np.full((Np, 3), 16.0 * len(levels["scale"]))             # 8 corners x 2 features per level
    out.inside, out.open, out.de, out.dsh = inside, op, de, dsh
    return out


def ray_sums64(ray, t, gx, gd, n_rays, mutate=None):
    """(go, goM, gdir, gdirM, n) per ray from the per-sample gradients of a canonical-order list: ray int [n] ascending, t fp32 [n]."""
    ray = np.asarray(ray, np.int64)
    t = np.asarray(t, np.float32).astype(np.float64)
    if mutate == "t_next":                                              # t_{k+1} for t_k (the list's next record)
        t = np.concatenate([t[1:], t[-1:]])
    gx, gd = np.asarray(gx, np.float64), np.asarray(gd, np.float64)
    go, goM, gr, grM = (np.zeros((n_rays, 3)) for _ in range(4))
    np.add.at(go, ray, gx)
    np.add.at(goM, ray, np.abs(gx))
    np.add.at(gr, ray, t[:, None] * gx + gd)
    np.add.at(grM, ray, np.abs(t[:, None] * gx) + np.abs(gd))
    return go, goM, gr, grM, np.bincount(ray, minlength=n_rays).astype(np.float64)
