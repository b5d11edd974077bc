"""fp64 restatement (numpy, no autograd) of the training backward of csrc/render_train.hip, element by element.

The rule, from that file's header.  For one ray with forward colour C (background included), g = dL/dC, kept samples k in ray order, each
with alpha_k (0 outside the model aabb), T_all over all kept samples, survivors = kept samples with T_all >= 1e-4, T_k over the survivors,
w_k = alpha_k T_k, colour c_k:
    dL/dc_k     = w_k g                         -> dL/do_k = w_k g c_k (1 - c_k)                    (the sigmoid)
    dL/dsigma_k = dt g . (T_{k+1} c_k - S_k),   S_k = C - sum_{j<=k} w_j c_j,   C = sum w c + bkgd (1 - sum w)
    dL/dh0      = dL/dsigma exp(min(h0 - 1, 15)),  0 outside the model aabb
then   d2 = relu'(h2) W3[0:3]^T do,   d1 = relu'(h1) W2^T d2,   dout[0] = dh0, dout[k] = sum_i W1[i][15 + k] d1[i]  (k = 1..15),
       dh = relu'(hd) W2d^T dout,     de = W1d^T dh,            table[corner of level l][f] += wt de[2 l + f]
and the five weight gradients are the sample sums of the outer products  do x h2,  d2 x h1,  d1 x xin,  dout x hd,  dh x enc.

Inputs.  `marched` is a march_restatement.Marched (the kept samples of every ray); `record` holds, per kept sample (arrays [Ns, .] or
broadcastable [1, .]), the forward's fp16 values enc [32], hd [64], raw [16], xin [32] (the colour net's input row), h1 [64], h2 [64], c [3],
and x [Ns,3], the fp32 sample positions x = fl(o + fl(t d)), t = fl(t_min + fl((n + 1/2) dt)) (march_restatement documents that rule;
sample_positions below forms them).  a, q: a sample's alpha and 1 - alpha inside the model aabb, scalars (the flat field of
tests/render_bwd_cases.py: the kernel's own fp32 values) or per kept sample.  Corner indices and weights are those of
tests/ngp_grad_restatement.py with coords = np.float32: u, pos = u scale + 1/2 and w = pos - floor(pos) are formed in fp32 as the kernel forms
them (they decide the cell), everything after them in fp64.

Every gradient element comes with M, the same sum with every term replaced by its absolute value down to the finest terms (T c, C's own
terms sum w c and bkgd (1 + sum w), sum_{j<=k} w_j c_j are separate terms of dL/dsigma), and n, the number of non-zero terms accumulated into
it: the rounding bound of tests/test_hip_render_bwd_fp64.py is (C + n) 2^-24 M.

Not observable here: the clamp of trunc_exp at h0 - 1 > 15.  A sample that saturated has alpha = 1 in fp32, so everything behind it is
cut and its own dL/dsigma multiplies T_{k+1} = 0 and S_k = 0: the clamp cannot be seen through this path.

`mutate` names one deliberate error (MUTATIONS): tests/test_render_bwd_host.py shows that each moves an element beyond the GPU test's bound."""
import numpy as np

import ngp_grad_restatement as GR

EPS = 1e-4
MUTATIONS = ("T_k", "no_bkgd", "no_1mc", "w3_rows", "cols_14", "mask_hd", "mask_h1", "mask_h2", "feat_swap", "scale_101", "corner7", "primes", "dh0_outside", "col31")
MATRICES = ("d1", "d2", "c1", "c2", "c3")             # density W1 [64,32], W2 [16,64]; colour W1 [64,32], W2 [64,64], W3 rows 0..2 [3,64]


def levels_of(rows):
    """oracle.ngp_oracle.level_table()[0] as the dict of arrays ngp_grad_restatement reads."""
    return {"offset": np.array([r["offset"] for r in rows], np.int64), "size": np.array([r["size"] for r in rows], np.uint32),
            "res": np.array([r["res"] for r in rows], np.uint32), "scale": np.array([r["scale"] for r in rows], np.float32),
            "hashed": np.array([r["hashed"] for r in rows], np.uint32)}


def sample_positions(o, d, tmin32, marched, dt):
    """x fp32 [Ns,3] of the kept samples, every operation rounded to fp32 as the kernel's march rounds it."""
    f = np.float32
    ray = marched.ray
    t = (tmin32.astype(f)[ray] + ((marched.n_idx.astype(f) + f(0.5)) * f(dt)).astype(f)).astype(f)
    return (o.astype(f)[ray] + (t[:, None] * d.astype(f)[ray]).astype(f)).astype(f)


class Result:
    """val / M / n per matrix (dicts keyed by MATRICES), the table in sparse form (t_idx: sorted flat element indices into the table part
    of mlp_base.params, t_val, t_M, t_n, t_level), firm [R], survivors [Ns], and per level the number of entries reached from two cells."""


def _index(cx, cy, cz, res, size, hashed, p1, p2):
    cx, cy, cz = cx.astype(np.uint32), cy.astype(np.uint32), cz.astype(np.uint32)
    with np.errstate(over="ignore"):
        idx = (cx ^ (cy * p1) ^ (cz * p2)) if hashed else (cx + cy * np.uint32(res) + cz * np.uint32(res) * np.uint32(res))
    return (idx % np.uint32(size)).astype(np.int64)


def backward64(record, weights, marched, a, q, g_rgb, bkgd, dt, levels, model_aabb, mutate=None, eps=EPS):
    assert mutate is None or mutate in MUTATIONS
    m = marched
    Ns, R = len(m.n_idx), len(m.ptr) - 1
    ray, inm = m.ray, m.in_model.astype(bool)
    dt = float(np.float32(dt))
    a_s = np.where(inm, np.broadcast_to(np.asarray(a, np.float64), (Ns,)), 0.0)
    q_s = np.where(inm, np.broadcast_to(np.asarray(q, np.float64), (Ns,)), 1.0)
    g_rgb, bk = np.asarray(g_rgb, np.float64), np.asarray(bkgd, np.float64)
    # ---- the forward sweep: survivors, T_k, T_{k+1}, w_k; firm = no early-stop decision within rounding of the threshold
    pos = np.arange(Ns) - m.ptr[:-1][ray]
    T_all, T_s, cnt, firm = np.ones(R), np.ones(R), np.zeros(R), np.ones(R, bool)
    surv, w, Tk, Tn = np.zeros(Ns, bool), np.zeros(Ns), np.zeros(Ns), np.zeros(Ns)
    order = np.argsort(pos, kind="stable")
    bounds = np.searchsorted(pos[order], np.arange(int(pos.max()) + 2 if Ns else 1))
    for p in range(len(bounds) - 1):
        sel = order[bounds[p]:bounds[p + 1]]
        r = ray[sel]
        firm[r] &= np.abs(T_all[r] - eps) > cnt[r] * 2.0 ** -22 * eps
        s = T_all[r] >= eps
        surv[sel], Tk[sel] = s, T_s[r]
        w[sel] = np.where(s, a_s[sel] * T_s[r], 0.0)
        T_all[r] = T_all[r] * q_s[sel]
        cnt[r] += inm[sel]
        T_s[r] = np.where(s, T_s[r] * q_s[sel], T_s[r])
        Tn[sel] = T_s[r]
    c = np.broadcast_to(np.asarray(record["c"], np.float64), (Ns, 3))
    wc = w[:, None] * c
    opac = np.bincount(ray, weights=w, minlength=R)
    acc = np.stack([np.bincount(ray, weights=wc[:, k], minlength=R) for k in range(3)], 1)
    C = acc + (0.0 if mutate == "no_bkgd" else bk[None] * (1.0 - opac[:, None]))
    CM = acc + np.abs(bk)[None] * (1.0 + opac[:, None])
    cum = np.cumsum(wc, axis=0)
    before = np.concatenate([np.zeros((1, 3)), cum])[m.ptr[:-1]]                 # the running sum at the start of each ray
    cum = cum - before[ray]
    g = g_rgb[ray]
    Tuse = (Tk if mutate == "T_k" else Tn)[:, None]
    dsig = dt * (g * (Tuse * c - (C[ray] - cum))).sum(1)
    dsigM = dt * (np.abs(g) * (Tuse * c + CM[ray] + cum)).sum(1)
    raw = np.broadcast_to(np.asarray(record["raw"], np.float64), (Ns, 16))
    ex = np.exp(np.minimum(raw[:, 0] - 1.0, 15.0))
    gate = surv & (inm | (mutate == "dh0_outside"))
    dh0, dh0M = np.where(gate, dsig * ex, 0.0), np.where(gate, dsigM * ex, 0.0)
    dO = w[:, None] * g * c * (1.0 if mutate == "no_1mc" else (1.0 - c))
    # ---- the chain, value and absolute value side by side
    W = {k: np.asarray(weights[k], np.float64) for k in MATRICES}
    rec = {k: np.broadcast_to(np.asarray(record[k], np.float64), (Ns, np.asarray(record[k]).shape[-1])) for k in ("enc", "hd", "xin", "h1", "h2")}
    mask = {k: rec[k] > 0 for k in ("hd", "h1", "h2")}

    def gated(layer, pre, preM):
        """relu'(layer) applied to the gradient arriving at it; mutation mask_<layer>: the mask of one unit inverted, the first unit at which
        a gradient arrives (a unit nothing reaches would show nothing)."""
        mk = mask[layer]
        if mutate == "mask_" + layer:
            reached = preM.any(axis=0)
            on = reached & mk.any(axis=0)                              # an active unit if there is one: switching it off changes live elements
            mk = mk ^ (np.arange(64) == int(np.argmax(on if on.any() else reached)))[None]
        return pre * mk, preM * mk

    w3 = W["c3"][[1, 0, 2]] if mutate == "w3_rows" else W["c3"][:3]
    cols = slice(15, 30) if mutate == "cols_14" else slice(16, 31)
    out = Result()
    out.val, out.M, out.n = {}, {}, {}

    def outer(name, A, Aabs, X):
        out.val[name], out.M[name] = A.T @ X, Aabs.T @ np.abs(X)
        out.n[name] = (Aabs != 0).astype(np.float64).T @ (X != 0).astype(np.float64)

    dOM = np.abs(dO)
    outer("c3", dO, dOM, rec["h2"])
    d2, d2M = gated("h2", dO @ w3, dOM @ np.abs(w3))
    outer("c2", d2, d2M, rec["h1"])
    d1, d1M = gated("h1", d2 @ W["c2"], d2M @ np.abs(W["c2"]))
    xin = rec["xin"].copy()
    if mutate == "col31":
        xin[:, 31] = 0.0
    outer("c1", d1, d1M, xin)
    dout, doutM = np.zeros((Ns, 16)), np.zeros((Ns, 16))
    dout[:, 0], doutM[:, 0] = dh0, dh0M
    dout[:, 1:], doutM[:, 1:] = d1 @ W["c1"][:, cols], d1M @ np.abs(W["c1"][:, cols])
    outer("d2", dout, doutM, rec["hd"])
    dh, dhM = gated("hd", dout @ W["d2"], doutM @ np.abs(W["d2"]))
    outer("d1", dh, dhM, rec["enc"])
    de, deM = dh @ W["d1"], dhM @ np.abs(W["d1"])
    # ---- the table: wt de[2 l + f] at the 8 corners of every level
    live = np.nonzero(deM.any(axis=1))[0]
    x = np.asarray(record["x"], np.float32)[live]
    de, deM = de[live], deM[live]
    u, _ = GR.unit_cube(x, model_aabb, np.float32)
    p1, p2 = (GR.P2, GR.P1) if mutate == "primes" else (GR.P1, GR.P2)
    parts, out.collisions = [], []
    for l in range(len(levels["scale"])):
        gcell, wf = GR.level_cells(u, levels["scale"][l], np.float32)
        e0, e1, m0, m1 = de[:, 2 * l], de[:, 2 * l + 1], deM[:, 2 * l], deM[:, 2 * l + 1]
        if mutate == "feat_swap" and l == 3:
            e0, e1 = e1, e0
        if mutate == "scale_101" and l == 5:
            e0, e1 = 1.01 * e0, 1.01 * e1
        es, vs, ms, keys = [], [], [], []
        for corner in range(8):
            if mutate == "corner7" and l == 15 and corner == 7:
                continue
            b = [(corner >> k) & 1 for k in range(3)]
            cc = [gcell[:, k] + np.uint32(b[k]) for k in range(3)]
            idx = _index(cc[0], cc[1], cc[2], levels["res"][l], levels["size"][l], levels["hashed"][l], p1, p2)
            wt = np.prod(np.stack([wf[:, k] if b[k] else 1.0 - wf[:, k] for k in range(3)], 1), axis=1)
            flat = 2 * (int(levels["offset"][l]) + idx)
            es += [flat, flat + 1]
            vs += [wt * e0, wt * e1]
            ms += [wt * m0, wt * m1]
            keys.append((idx << 40) | (cc[0].astype(np.int64) | (cc[1].astype(np.int64) << 13) | (cc[2].astype(np.int64) << 26)))
        e, v, mm = np.concatenate(es), np.concatenate(vs), np.concatenate(ms)
        uq, inv = np.unique(e, return_inverse=True)
        inv = inv.reshape(-1)
        M = np.bincount(inv, weights=mm, minlength=len(uq))
        keep = M > 0
        parts.append((uq[keep], np.bincount(inv, weights=v, minlength=len(uq))[keep], M[keep],
                      np.bincount(inv, weights=(mm > 0).astype(np.float64), minlength=len(uq))[keep], np.full(int(keep.sum()), l)))
        pairs = np.unique(np.concatenate(keys)) >> 40                                # one (entry, cell) pair each
        out.collisions.append(int((np.bincount(np.unique(pairs, return_inverse=True)[1].reshape(-1)) > 1).sum()) if len(pairs) else 0)
    out.t_idx, out.t_val, out.t_M, out.t_n, out.t_level = (np.concatenate([p[k] for p in parts]) for k in range(5))
    out.firm, out.surv = firm, surv
    return out
