"""fp64 restatement (numpy, no autograd) of the sample list of csrc/render_samples.hip and of its per-sample gradient rule.

The record.  A ray's kept samples (tests/march_restatement.Marched: ray, t_mid, in_model, in ray order) with alpha_k (0 outside the model
aabb) and colour c_k: T_all runs over all kept samples, a sample SURVIVES iff T_all >= 1e-4, T_s and w_k = alpha_k T_s over the survivors.
Survivor number ord of ray r is recorded as
    ray, ord, t = t_mid, T_next = T_s after the sample, w, c, P = sum_{j<=k} w_j c_j, Pd = sum_{j<=k} w_j t_j
and the ray's outputs are C = P_last + bkgd (1 - O), O = sum w, D = Pd_last.

The rule (csrc/render_samples.hip, ngp_samples_grad_kernel), g_C [R,3], g_O [R], g_D [R] the upstream gradients of a ray:
    dL/dc_k     = w_k g_C
    dL/dsigma_k = dt ( sum_ch g_C[ch] (T_next c_k[ch] - (C[ch] - P_k[ch]))  +  g_O (1 - O)  +  g_D (T_next t_k - (D - Pd_k)) )
from dw_k/dsigma_k = dt T_{k+1}, dw_j/dsigma_k = -dt w_j (j > k) and dO/dsigma_k = dt T_end = dt (1 - O).  Kept samples that do not
survive get nothing.  Every dL/dsigma comes with M, the same sum with every term replaced by its absolute value down to the terms the kernel
forms (T c, C, P; 1, O; T t, D, Pd), and n, the number of non-zero terms accumulated.

`mutate` names one deliberate error (MUTATIONS); tests/test_render_samples_host.py shows that each is seen.  With g_C alone the rule is
tests/render_bwd_restatement.backward64's dsig (that module is imported, not edited); whole_backward64 feeds the per-sample gradients to
tests/field_points_restatement.backward64 for the rest of the chain."""
import numpy as np

import field_points_restatement as FP
import render_bwd_cases as B          # noqa: F401  (the planted field and ray sets these records are built on)
import render_bwd_restatement as RB

EPS = RB.EPS
MUTATIONS = ("T_k", "O_for_1mO", "D_for_DmPd", "t_next", "no_bkgd", "no_w", "nonsurvivors")


class Records:
    """Per survivor (canonical order: ascending ray, then ord): ray, ord, kept (index into the kept samples), t, T_k, T_next, w, c [.,3],
    P [.,3], Pd; per ray: C [R,3], O [R], D [R], count [R]; surv [Ns] over the kept samples; firm [R] (no early-stop decision within
    rounding of the threshold)."""


def records64(ray, t_mid, alpha, c, bkgd, n_rays, in_model=None, q=None, eps=EPS):
    """ray [Ns] ascending (kept samples in ray order), t_mid [Ns], alpha [Ns] (or a scalar), c [Ns,3] (or broadcastable); q: the factor 1 - alpha of
    the transmittances where it is not the fp64 difference (the kernel's own fp32 value of 1 - a on the flat field), 1 outside the model aabb."""
    ray = np.asarray(ray, np.int64)
    Ns, R = len(ray), int(n_rays)
    t_mid = np.asarray(t_mid, np.float64)
    a = np.broadcast_to(np.asarray(alpha, np.float64), (Ns,)).copy()
    if in_model is not None:
        a = np.where(np.asarray(in_model, bool), a, 0.0)
    q = 1.0 - a if q is None else np.where(a != 0, np.broadcast_to(np.asarray(q, np.float64), (Ns,)), 1.0)
    c = np.broadcast_to(np.asarray(c, np.float64), (Ns, 3))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(ray, minlength=R))]).astype(np.int64)
    pos = np.arange(Ns) - ptr[:-1][ray]
    T_all, T_s, cnt, firm = np.ones(R), np.ones(R), np.zeros(R), np.ones(R, bool)
    P, Pd, ords = np.zeros((R, 3)), np.zeros(R), np.zeros(R, np.int64)
    surv = np.zeros(Ns, bool)
    out = {k: np.zeros(Ns) for k in ("T_k", "T_next", "w", "Pd")}
    out["P"], out["ord"] = np.zeros((Ns, 3)), np.zeros(Ns, np.int64)
    order = np.argsort(pos, kind="stable")
    bounds = np.searchsorted(pos[order], np.arange(int(pos.max()) + 2 if Ns else 1))
    for p in range(len(bounds) - 1):
        sel = order[bounds[p]:bounds[p + 1]]                           # the p-th kept sample of every ray that has one (a ray at most once)
        r = ray[sel]
        firm[r] &= np.abs(T_all[r] - eps) > cnt[r] * 2.0 ** -22 * eps
        s = T_all[r] >= eps
        surv[sel] = s
        T_all[r] *= q[sel]
        cnt[r] += a[sel] != 0
        sel, r = sel[s], r[s]
        out["T_k"][sel] = T_s[r]
        w = a[sel] * T_s[r]
        T_s[r] = T_s[r] * q[sel]
        P[r] += w[:, None] * c[sel]
        Pd[r] += w * t_mid[sel]
        out["T_next"][sel], out["w"][sel], out["P"][sel], out["Pd"][sel], out["ord"][sel] = T_s[r], w, P[r], Pd[r], ords[r]
        ords[r] += 1
    rec = Records()
    k = np.nonzero(surv)[0]
    rec.kept, rec.ray, rec.ord, rec.t, rec.c = k, ray[k], out["ord"][k], t_mid[k], c[k].copy()
    rec.T_k, rec.T_next, rec.w, rec.P, rec.Pd = out["T_k"][k], out["T_next"][k], out["w"][k], out["P"][k], out["Pd"][k]
    rec.O = np.bincount(rec.ray, weights=rec.w, minlength=R)
    rec.bkgd = np.asarray(bkgd, np.float64)
    rec.C = P + rec.bkgd[None] * (1.0 - rec.O[:, None])
    rec.D, rec.count, rec.surv, rec.firm = Pd, ords, surv, firm
    rec.all_ray, rec.all_t = ray, t_mid
    return rec


def planted_records(p, case, a, q=None):
    """The records of the planted flat field (tests/render_bwd_cases.planted) on a ray set, from the kept sets of case.ref
    (tests/march_restatement.py): alpha = a inside the model aabb (the kernel's own fp32 value), 0 outside, q = the kernel's fp32 value of
    1 - a (render_bwd_restatement.backward64's a, q), colour p["c"]."""
    m = case.ref
    return records64(m.ray, m.t_mid, a, p["c"][None], B.BKGD, len(m.ptr) - 1, in_model=m.in_model, q=q)


def sample_grads64(rec, g_rgb, g_opacity, g_depth, dt, mutate=None):
    """(g_sigma [n], g_c [n,3], M [n], n_terms [n]) of the records; each upstream gradient [R,..] or None (zeros).  With mutate ==
    "nonsurvivors" the returned arrays run over ALL kept samples (rec.surv says which survived), the opacity term given to every one."""
    assert mutate is None or mutate in MUTATIONS
    dt = float(np.float32(dt))
    r = rec.ray
    n = len(r)
    T = (rec.T_k if mutate == "T_k" else rec.T_next)
    C = rec.C - (rec.bkgd[None] * (1.0 - rec.O[:, None]) if mutate == "no_bkgd" else 0.0)
    g_sigma, M, cnt, g_c = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, 3))
    if g_rgb is not None:
        g = np.asarray(g_rgb, np.float64)[r]
        g_sigma += (g * (T[:, None] * rec.c - (C[r] - rec.P))).sum(1)
        CM = np.abs(rec.C[r])
        M += (np.abs(g) * (np.abs(T[:, None] * rec.c) + CM + np.abs(rec.P))).sum(1)
        cnt += 3.0 * (g != 0).sum(1)
        g_c = g if mutate == "no_w" else rec.w[:, None] * g
    if g_opacity is not None:
        go = np.asarray(g_opacity, np.float64)[r]
        g_sigma += go * (rec.O[r] if mutate == "O_for_1mO" else 1.0 - rec.O[r])
        M += np.abs(go) * (1.0 + rec.O[r])
        cnt += 2.0 * (go != 0)
    if g_depth is not None:
        gd = np.asarray(g_depth, np.float64)[r]
        t = rec.t
        if mutate == "t_next":                                          # the next kept sample's t_mid (the ray's last: one step on)
            nxt = np.minimum(rec.kept + 1, len(rec.all_t) - 1)
            t = np.where(rec.all_ray[nxt] == r, rec.all_t[nxt], rec.t + dt)
        g_sigma += gd * (T * t - (rec.D[r] if mutate == "D_for_DmPd" else rec.D[r] - rec.Pd))
        M += np.abs(gd) * (np.abs(T * t) + np.abs(rec.D[r]) + np.abs(rec.Pd))
        cnt += 3.0 * (gd != 0)
    g_sigma, M = dt * g_sigma, dt * M
    if mutate == "nonsurvivors":
        Ns = len(rec.surv)
        full, full_c = np.zeros(Ns), np.zeros((Ns, 3))
        full[rec.kept], full_c[rec.kept] = g_sigma, g_c
        if g_opacity is not None:
            dead = ~rec.surv
            full[dead] = dt * np.asarray(g_opacity, np.float64)[rec.all_ray[dead]] * (1.0 - rec.O[rec.all_ray[dead]])
        return full, full_c, None, None
    return g_sigma, g_c, M, cnt


def whole_backward64(rec, record, weights, g_rgb, g_opacity, g_depth, dt, levels, model_aabb):
    """The whole backward on the records: the rule above, then tests/field_points_restatement.backward64 (dL/dh0 = dL/dsigma exp(min(h0 - 1,
    15)) inside the model aabb, the two nets, the table).  `record`: the forward record per survivor (enc, hd, raw, xin, h1, h2, c, x).  Returns
    (val, absolute): two render_bwd_restatement.Result; val.val the gradients, absolute.M the sums of absolute terms and absolute.n the
    accumulated terms (the same chain fed with M of dL/dsigma and |dL/dc|)."""
    g_sigma, g_c, M, _ = sample_grads64(rec, g_rgb, g_opacity, g_depth, dt)
    val = FP.backward64(record, weights, g_sigma, g_c if g_rgb is not None else None, levels, model_aabb)
    absolute = FP.backward64(record, weights, M, np.abs(g_c) if g_rgb is not None else None, levels, model_aabb)
    return val, absolute
