"""CPU restatement of the arithmetic of csrc/attention.hip (forward, dQ, dK/dV; head dim 32 with V [Nk,32] and the 256-channel `xyz` form with
V = fp32 coordinates), tile by tile as the kernels do it, in plain torch: no HIP.  It is the yardstick of tests/test_hip_attention.py (a kernel's
error against fp64 may be 4 x this restatement's, see `bound`) and, through its defect switches, the proof in tests/test_attention_host.py that the
case list and the tolerances tell a subtly wrong kernel from a right one.

What is restated:
  * keys (dQ, forward) and queries (dK/dV) are streamed 64 rows at a time, rows past the end are ZERO (the kernels' LDS tiles);
  * forward: online max and sum in the log2 domain (c2 = scale * log2 e folded into the exponent's fused multiply-add), the tail-key mask
    in the last tile only, the running output rescaled by alpha = exp2(m_old - m_new), one division at the end, lse = (m + log2 l) ln 2;
  * backward: p = exp2(s c2 - lse log2 e), dvec = rowsum(dO * O) from the STORED O, dS = p (dP - dvec), the softmax scale applied once at the
    end to dQ and dK; dQ zeroes p of the keys past Nk in the last tile (their K rows are zero, but p = exp2(-lse2) is +inf once lse < -88.7);
  * bf16 mode: operands are bf16 values (held in fp32 here), products accumulate in fp32, P and dS are rounded to bf16 before the second
    product, outputs are rounded to bf16; the xyz value path (coordinates, out, dO) stays fp32.
What is not: the order of the additions inside an MFMA and across the four lane groups, and the hardware exp2 / log2 — the factor 4 of `bound`.

Layout: q, k [H, R, D]; v [H, R, 32] (or xyz [R, 3]); go [H, R, 32] (or [H, R, 3]); `table` = [(q_start, q_len, kv_start, kv_len), ...] rows of the
shared row space, as the varlen entry points take it.  Rows no problem owns stay NaN in the results."""
import math

import torch

LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)
LN2 = torch.tensor(0.6931471805599453, dtype=torch.float32)
TILE = 64

DEFECTS = ("no_tail_mask", "no_alpha", "dq_scale_twice", "dq_scale_none", "v_ignores_kv_start", "dkv_dvec_row0", "dkv_lse_row0", "dq_no_tail_mask")


def _rb(x, mode):
    """Round to the operand dtype of `mode` (kept in fp32)."""
    return x.bfloat16().float() if mode == "bf16" else x


def _fma_exp2(s, c2, sub):
    """exp2(fma(s, c2, -sub)) in fp32: the product of two fp32 values is exact in fp64."""
    return torch.exp2((s.double() * c2.double() - sub.double()).float())


def _dot(a, b, mode):
    """a [H, n, C] . b [H, m, C]^T -> [H, n, m] in fp32, the channels taken in the order of the kernels' first products: bf16 = one 16x16x32
    MFMA per 32 channels; fp32 = eight 16x16x4 MFMAs per 32 channels, the e-th over channels {8g + e, g = 0..3} (common `mma`).  The sum
    inside one MFMA is taken as exact (fp64 here), its result is rounded to fp32 when it joins the accumulator."""
    H, n, C = a.shape
    acc = torch.zeros(H, n, b.shape[1])
    a64, b64 = a.double(), b.double()
    for c0 in range(0, C, 32):
        groups = [list(range(c0, min(c0 + 32, C)))] if mode == "bf16" or C < 32 else [[c0 + 8 * g + e for g in range(4)] for e in range(8)]
        for idx in groups:
            acc = (acc.double() + a64[:, :, idx] @ b64[:, :, idx].transpose(1, 2)).float()
    return acc


def _tile(x, r0, n):
    """Rows r0 .. r0+63 of x [H, n, C]; rows past n are zero."""
    t = x[:, r0:min(r0 + TILE, n)]
    if t.shape[1] < TILE:
        t = torch.cat([t, torch.zeros(x.shape[0], TILE - t.shape[1], x.shape[2], dtype=x.dtype)], 1)
    return t


def run(q, k, v, go, table, scale, mode, xyz, **defects):
    """-> dict(o, lse, dvec, dq, dk, dv) (dv None for xyz).  `defects`: any of DEFECTS=True seeds that one defect."""
    for name in defects:
        assert name in DEFECTS, name
    df = lambda name: bool(defects.get(name, False))
    H, R, D = q.shape
    f32 = torch.float32
    scale32 = torch.tensor(scale, dtype=f32)
    c2 = scale32 * LOG2E
    q, k, go = q.float(), k.float(), go.float()
    vh = v.float()[None].expand(H, -1, -1) if xyz else v.float()     # [H, R, 3 or 32]
    DV = vh.shape[2]
    nan = float("nan")
    res = {"o": torch.full((H, R, DV), nan), "lse": torch.full((H, R), nan), "dvec": torch.full((H, R), nan),
           "dq": torch.full((H, R, D), nan), "dk": torch.full((H, R, D), nan), "dv": None if xyz else torch.full((H, R, DV), nan)}
    rnd = (lambda x: x) if xyz else (lambda x: _rb(x, mode))        # rounding of the VALUE path: none for xyz
    rp = lambda x: _rb(x, mode)                                     # P / dS feeding an MFMA
    for (qs, nq, ks, nk) in table:
        Q, K, dO = q[:, qs:qs + nq], k[:, ks:ks + nk], go[:, qs:qs + nq]
        vs = 0 if df("v_ignores_kv_start") else ks
        V = vh[:, vs:vs + nk]
        # ------------------------------------------------------------------ forward
        m = torch.full((H, nq), -math.inf)
        l = torch.zeros(H, nq)
        o = torch.zeros(H, nq, DV)
        for k0 in range(0, nk, TILE):
            kt, vt = _tile(K, k0, nk), _tile(V, k0, nk)
            s = _dot(Q, kt, mode)
            if k0 + TILE > nk and not df("no_tail_mask"):
                s[:, :, nk - k0:] = -math.inf
            mx = s.max(dim=2).values * c2
            mn = torch.maximum(m, mx)
            alpha = torch.exp2(m - mn)
            p = _fma_exp2(s, c2, mn[:, :, None])
            l = l * alpha + p.sum(dim=2)
            m = mn
            if not df("no_alpha"):
                o = o * alpha[:, :, None]
            o = o + (p if xyz else rp(p)) @ vt
        o = rnd(o * (1.0 / l)[:, :, None])
        lse = (m + torch.log2(l)) * LN2
        res["o"][:, qs:qs + nq], res["lse"][:, qs:qs + nq] = o, lse
        # ------------------------------------------------------------------ dQ
        lse2 = lse * LOG2E
        dvec = (dO * o).sum(dim=2)
        res["dvec"][:, qs:qs + nq] = dvec
        dq = torch.zeros(H, nq, D)
        for k0 in range(0, nk, TILE):
            kt, vt = _tile(K, k0, nk), _tile(V, k0, nk)
            p = _fma_exp2(_dot(Q, kt, mode), c2, lse2[:, :, None])
            if k0 + TILE > nk and not df("dq_no_tail_mask"):
                p[:, :, nk - k0:] = 0.0
            ds = p * (_dot(dO, vt, mode) - dvec[:, :, None])
            dq = dq + rp(ds) @ kt
        if not df("dq_scale_none"):
            dq = dq * scale32
        if df("dq_scale_twice"):
            dq = dq * scale32
        res["dq"][:, qs:qs + nq] = _rb(dq, mode)
        # ------------------------------------------------------------------ dK, dV
        dk = torch.zeros(H, nk, D)
        dv = torch.zeros(H, nk, DV)
        for q0 in range(0, nq, TILE):
            qt, gt = _tile(Q, q0, nq), _tile(dO, q0, nq)
            lt, dt = _tile(lse2[:, :, None], q0, nq)[:, :, 0], _tile(dvec[:, :, None], q0, nq)[:, :, 0]
            if q0 + TILE >= nq:
                if df("dkv_lse_row0"):
                    lt = lt[:, :1].expand(-1, TILE)
                if df("dkv_dvec_row0"):
                    dt = dt[:, :1].expand(-1, TILE)
            # query rows past Nq: Q, dO, lse, dvec are zero, so p = 1 and dS = 0 multiply zero rows
            p = _fma_exp2(_dot(qt, K, mode), c2, lt[:, :, None])                  # [H, 64, nk]
            ds = p * (_dot(gt, V, mode) - dt[:, :, None])
            dk = dk + rp(ds).transpose(1, 2) @ qt
            dv = dv + rp(p).transpose(1, 2) @ gt
        res["dk"][:, ks:ks + nk] = _rb(dk * scale32, mode)
        if not xyz:
            res["dv"][:, ks:ks + nk] = _rb(dv, mode)
    return res


def reference(q, k, v, go, table, scale, xyz):
    """Direct fp64 softmax(Q K^T s) V and its autograd gradients, per problem (all heads / layers at once, each independent)."""
    H, R, D = q.shape
    q, k, go = q.double(), k.double(), go.double()
    vh = v.double()[None].expand(H, -1, -1) if xyz else v.double()
    DV = vh.shape[2]
    nan = float("nan")
    f64 = torch.float64
    res = {"o": torch.full((H, R, DV), nan, dtype=f64), "lse": torch.full((H, R), nan, dtype=f64), "dq": torch.full((H, R, D), nan, dtype=f64),
           "dk": torch.full((H, R, D), nan, dtype=f64), "dv": None if xyz else torch.full((H, R, DV), nan, dtype=f64)}
    for (qs, nq, ks, nk) in table:
        Q = q[:, qs:qs + nq].clone().requires_grad_(True)
        K = k[:, ks:ks + nk].clone().requires_grad_(True)
        V = vh[:, ks:ks + nk].clone().requires_grad_(True)
        s = Q @ K.transpose(1, 2) * scale
        o = torch.softmax(s, dim=2) @ V
        o.backward(go[:, qs:qs + nq])
        res["o"][:, qs:qs + nq], res["lse"][:, qs:qs + nq] = o.detach(), torch.logsumexp(s.detach(), dim=2)
        res["dq"][:, qs:qs + nq], res["dk"][:, ks:ks + nk] = Q.grad, K.grad
        if not xyz:
            res["dv"][:, ks:ks + nk] = V.grad
    return res


# ------------------------------------------------------------------------------------------------------- the error measure and its bound
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
CAP = {"fp32": 2e-5, "bf16": 3e-2}     # what the project's attention tests assert already: no bound may be looser


def rows_of(name, prob):
    qs, nq, ks, nk = prob
    return (qs, nq) if name in ("o", "lse", "dvec", "dq") else (ks, nk)


def zero_scales(q, k, v, go, scale):
    """The size of the terms that cancel where a gradient is exactly zero in fp64 (one key: p = 1, dS = dO.v - dO.o = 0; q = 0: dK = 0 * dS):
    |dS| <= dv |dO| |v|, dQ = scale dS K, dK = scale dS Q.  The denominator of the error measure for such a problem."""
    s = scale * go.shape[-1] * float(go.abs().max()) * float(v.abs().max())
    return {"dq": s * float(k.abs().max()), "dk": s * float(q.abs().max())}


def errors(got, ref, table, names=OUTPUTS, zero_scale=None):
    """{output: [error of problem p, head h ...]}: max |got - ref64| / max |ref64| over the rows the problem owns (every element); lse in
    absolute terms.  Where the reference is exactly zero the denominator is zero_scale[output] (see zero_scales); where that is zero too
    (dK at q = 0) the result must be exactly zero: error 0 or inf.  Non-finite results give inf."""
    out = {}
    for name in names:
        if ref.get(name) is None:
            continue
        es = []
        for prob in table:
            r0, n = rows_of(name, prob)
            for h in range(ref[name].shape[0]):
                g, r = got[name][h, r0:r0 + n].double(), ref[name][h, r0:r0 + n]
                assert torch.isfinite(r).all(), "the fp64 reference itself is not finite"
                if not torch.isfinite(g).all():
                    es.append(math.inf)
                    continue
                d, den = float((g - r).abs().max()), float(r.abs().max())
                if name == "lse":
                    es.append(d)
                elif den == 0.0:
                    zs = (zero_scale or {}).get(name, 0.0)
                    es.append(0.0 if d == 0.0 else (d / zs if zs > 0.0 else math.inf))
                else:
                    es.append(d / den)
        out[name] = es
    return out


def ulp_floor(name, mode, xyz, ref, table):
    """What two correct computations may differ by, from the number formats alone.  Measured on the MI355X, six cases of the list need more than
    4 x the restatement's error because the restatement's own error is far below these figures there (it was 'lucky'), each for one of two reasons:
      * lse (absolute; e.g. the peaked xyz cases in bf16: kernel 8.7e-6, restatement 2.0e-6 at |lse| ~ 43) passes through four fp32 roundings at its
        own size or 1.44 x it (the score, m = max * c2 in the log2 domain, m + log2 l, * ln 2): 3 ulp of the largest |lse|;
      * an fp32-stored output is the end of a chain of N / 4 (fp32 MFMA) .. N (VALU, xyz) additions into ONE fp32 accumulator, N = the keys (o, dq)
        or queries (dk, dv) of the problem, each rounding the running sum; the restatement sums a 64-row tile in one CPU matmul.  Random-walk growth:
        sqrt(N) ulp (1184x1170 dv in fp32: kernel 1.8e-6, restatement 4.2e-7, sqrt(1184) 2^-23 = 4.1e-6; 65x63 q = 0 xyz o: 1.5e-7 against 3.5e-8).
    bf16-stored outputs: one ulp, 2^-8 of the largest element (their fp32 accumulators are far below it)."""
    if name == "lse":
        return 3 * 2.0 ** -23 * max(1.0, float(ref["lse"][torch.isfinite(ref["lse"])].abs().max()))
    if mode == "bf16" and not (xyz and name == "o"):
        return 2.0 ** -8
    n = max(p[3] if name in ("o", "dq") else p[1] for p in table)
    return 2.0 ** -23 * math.sqrt(n)


def bound(name, mode, xyz, rest_err, ref, table):
    """The bound of one output of one case: 4 x the restatement's own error against fp64 on that case (the largest over its problems and heads;
    4 = a different order of additions inside the MFMA and across lane groups, and the hardware exp2), never below ulp_floor, never above what
    the project asserts already (CAP; lse, always fp32, takes the fp32 cap in both modes)."""
    cap = CAP["fp32"] if name == "lse" else CAP[mode]          # lse is stored in fp32 in both modes
    return min(cap, max(4.0 * max(rest_err[name]), ulp_floor(name, mode, xyz, ref, table)))


# ------------------------------------------------------------------------------------------------------- the case list
LENGTHS = (1, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 192, 193, 333, 1184)
# (Nq, Nk): every length as a query length and as a key length, 1 / 2 / >= 3 tiles on both sides, the four the issue names
SHAPES = [(1, 1), (1, 193), (193, 1), (1184, 1170), (3, 17), (15, 64), (16, 3), (17, 15), (63, 65), (64, 16), (65, 63), (127, 129), (128, 128),
          (129, 127), (192, 333), (193, 192), (333, 1184)]
# segment lengths for ProblemTable: (source, target) per pair.  A one-row set next to the longest; the max_len problem never first
TABLES = {"one_next_to_long": [(1, 1184), (65, 63)], "mixed": [(193, 128), (17, 333), (64, 129)], "small": [(3, 15), (16, 127), (192, 1)]}
REGIMES = ("unit", "shift_neg", "shift_pos", "peaked_last", "peaked_first", "qzero")


def single_table(nq, nk):
    """One cross problem: queries rows 0 .. nq-1, keys rows nq .. nq+nk-1 of a shared space (non-zero kv_start even here)."""
    return [(0, nq, nq, nk)]


def segs_tables(segs):
    """(self problems, cross problems, R) of ProblemTable(segs), restated on the host."""
    self_p, cross_p, off = [], [], 0
    for ns, nt in segs:
        s0, t0 = off, off + ns
        self_p += [(s0, ns, s0, ns), (t0, nt, t0, nt)]
        cross_p += [(s0, ns, t0, nt), (t0, nt, s0, ns)]
        off += ns + nt
    return self_p, cross_p, off


def case_list():
    """[(name, kind, table, R, regime)]; kind 'single' runs through the non-varlen wrappers, 'self' / 'cross' through the varlen ones."""
    cases = []
    for nq, nk in SHAPES:
        cases.append((f"{nq}x{nk}-unit", "single", single_table(nq, nk), nq + nk, "unit"))
    for regime, shapes in (("shift_neg", [(17, 15), (65, 63), (128, 129), (193, 333)]), ("shift_pos", [(17, 15), (65, 63), (128, 129), (193, 333)]),
                           ("peaked_last", [(63, 65), (129, 193)]), ("peaked_first", [(63, 65), (129, 193)]),
                           ("qzero", [(1, 193), (64, 16), (65, 63), (192, 333)])):
        for nq, nk in shapes:
            cases.append((f"{nq}x{nk}-{regime}", "single", single_table(nq, nk), nq + nk, regime))
    for tname, segs in TABLES.items():
        sp, cp, R = segs_tables(segs)
        cases.append((f"{tname}-self-unit", "self", sp, R, "unit"))
        cases.append((f"{tname}-cross-unit", "cross", cp, R, "unit"))
    sp, cp, R = segs_tables(TABLES["mixed"])
    for regime in ("shift_neg", "shift_pos", "peaked_last", "qzero"):
        cases.append((f"mixed-cross-{regime}", "cross", cp, R, regime))
    cases.append(("mixed-self-shift_neg", "self", sp, R, "shift_neg"))
    return cases


# The shared direction of the shifted and peaked regimes is the LAST channel, and the shift is split unevenly between q and k.  Both choices
# keep the problem well enough conditioned for the caps the project asserts (2e-5 / 3e-2), and both were measured with this restatement:
#   * a score of size 104 / scale (~590 raw at D = 32) rounds by ulp(590) * scale ~ 1e-5 in the exponent at EVERY fp32 addition made after the
#     shift term has entered the dot product.  In channel 0 every later partial sum pays it and any fp32 accumulation misses fp64 by 2 .. 6e-5 in
#     `o`; in the last channel the kernels (and _dot above) add it last: one rounding.
#   * dQ's shared channel is k_c * sum_j dS_j with sum_j dS_j = 0 in exact arithmetic: the rounding of dS (to bf16 by design) comes out
#     multiplied by |k_c|.  With q_c = k_c = 24.25 that alone is 3.5 .. 6.5e-2 of max |dQ| in bf16; with |k_c| = 4 it is 4 / 24.25 of that.
# q_c * k_c * scale = -+104.7 (D = 32, scale 1/sqrt 32) and -+104 (D = 256, scale 1/16); every value is exact in bf16.
SHIFT_Q = {32: 148.0, 256: 416.0}
SHIFT_K = 4.0
# peaked: the leading key's score is ~40 above the others (e^-40 ~ 4e-18: its probability is 1 to fp32 and fp64 alike); a smaller score than the
# shifted regimes' keeps lse (compared in ABSOLUTE terms, stored in fp32) at a size whose ulp is below the cap
PEAK_Q = {32: 64.0, 256: 160.0}
PEAK_K = {32: 3.5, 256: 4.0}
XYZ_SPREAD = 1.0e3


def make_inputs(table, R, regime, xyz, mode, H, seed):
    """q, k [H,R,D], v ([H,R,32] or xyz [R,3]), go, scale — fp32 tensors already rounded to the operand dtype of `mode`.
    shift_neg / shift_pos: the last channel of every q row is SHIFT_Q and of every k row -+SHIFT_K: every score moves by -+104 exactly, so the
    fp64 lse of every row is below -90 / above +90.  peaked_*: the last channel of q is PEAK_Q, of the last / first key of every problem PEAK_K, of
    the other keys 0.  qzero: q = 0.  xyz coordinates are ~1e3 (they must never pass through bf16); dO is unit random."""
    D = 256 if xyz else 32
    g = torch.Generator().manual_seed(seed)
    scale = 1.0 / math.sqrt(D)
    q, k = torch.randn(H, R, D, generator=g), torch.randn(H, R, D, generator=g)
    v = torch.randn(R, 3, generator=g) * XYZ_SPREAD if xyz else torch.randn(H, R, 32, generator=g)
    go = torch.randn(H, R, 3 if xyz else 32, generator=g)
    c = D - 1
    if regime in ("shift_neg", "shift_pos"):
        q[:, :, c] = SHIFT_Q[D]
        k[:, :, c] = -SHIFT_K if regime == "shift_neg" else SHIFT_K
    elif regime in ("peaked_last", "peaked_first"):
        q[:, :, c] = PEAK_Q[D]
        k[:, :, c] = 0.0
        for prob in table:
            k[:, peaked_key(prob, regime), c] = PEAK_K[D]
    elif regime == "qzero":
        q.zero_()
    else:
        assert regime == "unit"
    q, k = _rb(q, mode), _rb(k, mode)
    if not xyz:
        v, go = _rb(v, mode), _rb(go, mode)
    return q, k, v, go, scale


def compared_outputs(regime, xyz):
    """The outputs with a relative measure against fp64.  peaked: dQ and dK are ~e^-40 of anything in fp64 (the leading key's probability is 1,
    dS = dO.(v - o) vanishes) and are checked in absolute terms instead; dV of the 32-channel form is ordinary (sum_i dO_i at the leading key)."""
    if regime.startswith("peaked"):
        return ("o", "lse") if xyz else ("o", "lse", "dv")
    return OUTPUTS


def peaked_key(prob, regime):
    qs, nq, ks, nk = prob
    return ks + (nk - 1 if regime == "peaked_last" else 0)
