"""fp64 restatement (numpy, no autograd) of the point-wise field backward of csrc/field_train.hip, element by element, in the
form of tests/render_bwd_restatement.backward64 with the ray part replaced by the two upstream gradients.

The rule.  Point i with forward record (fp16 values) enc [32], hd [64], raw [16], xin [32] = (fp16 SH4(d) | raw[1:16] | 1), h1 [64], h2 [64],
c [3] and position x (fp32), upstream gradients g_sigma, g_rgb:
    dL/dh0  = g_sigma exp(min(h0 - 1, 15)) inside the model aabb (strictly), 0 outside          dL/do = g_rgb c (1 - c)
    d2 = relu'(h2) W3[0:3]^T do,   d1 = relu'(h1) W2^T d2,   dout[0] = dh0, dout[k] = sum_i W1[i][15 + k] d1[i]  (k = 1..15),
    dh = relu'(hd) W2d^T dout,     de = W1d^T dh,            table[corner of level l][f] += wt de[2 l + f]
and the five weight gradients are the point sums of the outer products  do x h2,  d2 x h1,  d1 x xin,  dout x hd,  dh x enc.  The colour
gradient does not depend on the aabb (query_rgb does not); the encoding of a point outside is that of its clamped unit coordinates.

Corner indices and weights are those of tests/ngp_grad_restatement.py with coords = np.float32 (u, pos and w are formed in fp32 as the kernel
forms them: they decide the cell), everything after them in fp64.  Every element comes with M, the same sum with every term replaced by its
absolute value, and n, the number of non-zero terms accumulated into it: the bound of tests/test_hip_field_train.py is (C + n) 2^-24 M.

`mutate` names one deliberate error (MUTATIONS); tests/test_field_train_host.py shows that each moves an element beyond four times that bound."""
import numpy as np

import ngp_grad_restatement as GR
from render_bwd_restatement import MATRICES, Result, _index, levels_of   # noqa: F401  (the shared layout of the five matrices)

MUTATIONS = ("w3_rows", "mask_hd", "mask_h1", "mask_h2", "corner7", "primes", "exp_h0", "dh0_outside")


def forward_record(x, dirs, base, color, aabb):
    """The oracle's forward record of a general field at the points (oracle.ngp_oracle's arithmetic: fp32 sums between fp16 roundings), as fp64
    arrays, with the weights' fp16 values: (record, weights, inside)."""
    import torch
    from oracle import ngp_oracle as N
    x, dirs = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(dirs, dtype=torch.float32)
    base, color = torch.as_tensor(base, dtype=torch.float32), torch.as_tensor(color, dtype=torch.float32)
    aabb = torch.as_tensor(aabb, dtype=torch.float32)
    with torch.no_grad():
        u = (x - aabb[:3]) / (aabb[3:] - aabb[:3])
        inside = ((u > 0) & (u < 1)).all(-1)
        w1, w2, table = N.split_density_params(base)
        enc = N.hash_encode(u, N.f16(table))
        hd = N.f16(torch.relu(enc @ N.f16(w1).T))
        raw = N.f16(hd @ N.f16(w2).T)
        c1, c2, c3 = N.split_color_params(color)
        xin = torch.cat([N.f16(N.sh4((dirs + 1.0) / 2.0 * 2.0 - 1.0)), raw[:, 1:16]   # (query_rgb's own round trip through [0,1])
                        , torch.ones(len(x), 1)], 1)
        h1 = N.f16(torch.relu(xin @ N.f16(c1).T))
        h2 = N.f16(torch.relu(h1 @ N.f16(c2).T))
        o = N.f16(h2 @ N.f16(c3).T)[:, :3]
        s = torch.sigmoid(o)
        col = N.f16(s)
    record = {k: v.double().numpy() for k, v in dict(enc=enc, hd=hd, raw=raw, xin=xin, h1=h1, h2=h2, c=col, s=s).items()}
    record["x"] = x.numpy()
    f16w = lambda t: N.f16(t).double().numpy()
    return record, dict(d1=f16w(w1), d2=f16w(w2), c1=f16w(c1), c2=f16w(c2), c3=f16w(c3)), inside.numpy()


def backward64(record, weights, g_sigma, g_rgb, levels, model_aabb, mutate=None):
    """record: arrays [N, .] or broadcastable [1, .] (enc, hd, raw, xin, h1, h2, c) and x fp32 [N,3]; g_sigma [N] / g_rgb [N,3] or None (zeros).
    Returns a render_bwd_restatement.Result: val / M / n per matrix, the table in sparse form (t_idx, t_val, t_M, t_n, t_level), inside [N]."""
    assert mutate is None or mutate in MUTATIONS
    x = np.asarray(record["x"], np.float32)
    Np = len(x)
    gs = np.zeros(Np) if g_sigma is None else np.asarray(g_sigma, np.float64)
    gc = np.zeros((Np, 3)) if g_rgb is None else np.asarray(g_rgb, np.float64)
    u, inside = GR.unit_cube(x, model_aabb, np.float32)
    raw = np.broadcast_to(np.asarray(record["raw"], np.float64), (Np, 16))
    c = np.broadcast_to(np.asarray(record["c"], np.float64), (Np, 3))
    ex = np.exp(raw[:, 0]) if mutate == "exp_h0" else np.exp(np.minimum(raw[:, 0] - 1.0, 15.0))
    gate = inside | (mutate == "dh0_outside")
    dh0, dh0M = np.where(gate, gs * ex, 0.0), np.where(gate, np.abs(gs) * ex, 0.0)
    dO = gc * c * (1.0 - c)
    W = {k: np.asarray(weights[k], np.float64) for k in MATRICES}
    rec = {k: np.broadcast_to(np.asarray(record[k], np.float64), (Np, np.asarray(record[k]).shape[-1])) for k in ("enc", "hd", "xin", "h1", "h2")}
    mask = {k: rec[k] > 0 for k in ("hd", "h1", "h2")}

    def gated(layer, pre, preM):
        """relu'(layer) applied to the gradient arriving at it; mutation mask_<layer>: the mask of one unit inverted, an active unit at which a
        gradient arrives if there is one (a unit nothing reaches would show nothing)."""
        mk = mask[layer]
        if mutate == "mask_" + layer:
            reached = preM.any(axis=0)
            on = reached & mk.any(axis=0)
            mk = mk ^ (np.arange(64) == int(np.argmax(on if on.any() else reached)))[None]
        return pre * mk, preM * mk

    w3 = W["c3"][[1, 0, 2]] if mutate == "w3_rows" else W["c3"][:3]
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
    outer("c1", d1, d1M, rec["xin"])
    dout, doutM = np.zeros((Np, 16)), np.zeros((Np, 16))
    dout[:, 0], doutM[:, 0] = dh0, dh0M
    dout[:, 1:], doutM[:, 1:] = d1 @ W["c1"][:, 16:31], d1M @ np.abs(W["c1"][:, 16:31])
    outer("d2", dout, doutM, rec["hd"])
    dh, dhM = gated("hd", dout @ W["d2"], doutM @ np.abs(W["d2"]))
    outer("d1", dh, dhM, rec["enc"])
    de, deM = dh @ W["d1"], dhM @ np.abs(W["d1"])
    # ---- the table: wt de[2 l + f] at the 8 corners of every level
    live = np.nonzero(deM.any(axis=1))[0]
    u, de, deM = u[live], de[live], deM[live]
    p1, p2 = (GR.P2, GR.P1) if mutate == "primes" else (GR.P1, GR.P2)
    parts = []
    for l in range(len(levels["scale"])):
        gcell, wf = GR.level_cells(u, levels["scale"][l], np.float32)
        e0, e1, m0, m1 = de[:, 2 * l], de[:, 2 * l + 1], deM[:, 2 * l], deM[:, 2 * l + 1]
        es, vs, ms = [], [], []
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
        if not es or not len(live):
            continue
        e, v, mm = np.concatenate(es), np.concatenate(vs), np.concatenate(ms)
        uq, inv = np.unique(e, return_inverse=True)
        inv = inv.reshape(-1)
        M = np.bincount(inv, weights=mm, minlength=len(uq))
        keep = M > 0
        parts.append((uq[keep], np.bincount(inv, weights=v, minlength=len(uq))[keep], M[keep],
                      np.bincount(inv, weights=(mm > 0).astype(np.float64), minlength=len(uq))[keep], np.full(int(keep.sum()), l)))
    if parts:
        out.t_idx, out.t_val, out.t_M, out.t_n, out.t_level = (np.concatenate([p[k] for p in parts]) for k in range(5))
    else:
        out.t_idx, out.t_val, out.t_M, out.t_n, out.t_level = (np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.int64))
    out.inside = inside
    return out
