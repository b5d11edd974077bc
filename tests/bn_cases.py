"""BatchNorm and column-sum cases for tests/test_bn_host.py (no GPU) and tests/test_hip_bn_fp64.py (GPU): a seeded generator, the fp64
reference, the rounding-count bounds and the case table.  Imports without a GPU.

Operands.  x and dy are small integers (x in [-7, 8] plus a per-channel integer offset in [-4, 4], dy in [-7, 8]); the library is built with
-ffp-contract=off.  Every fp32 partial sum of x, x^2 and of the masked gradient g is then an exact integer below 2^24 (they are per chunk
of <= 512 rows, or per grid of V <= 512 rows, and continue in double: bn_finalize_kernel / bn_small_fwd_kernel `s1 += p.x`, `a1 += red[..]`),
and the kernels' `mean = s1 / V`, `var = s2 / V - mean * mean` are the very double expressions evaluated here.  EXACT (torch.equal):
mean_rstd[..., 0], var_keep, dbeta (accumulate = 0, or onto integers), dres outside ambiguous elements, the x a split-K forward writes
back, every column sum.

Everything else: a bound that counts roundings.  u = 2^-24, g_n = n u / (1 - n u) (n roundings compounded), bT = 2^-8 for a bf16 store
(8-bit significand, round to nearest even: `(__bf16)f` in csrc/common.h), 0 for fp32.  The issue that asked for these tests proposed
8u (|x sc| + |mean sc| + |beta| + |res|) + 2^-8 |y64| for y, (n32 + 8) u sum|g xhat| for dgamma and 8u (|g| + |c1| + |xhat c2|) for dx; the
counts below are this module's own reading of the same lines and differ where noted.  No constant here was fitted to a GPU result.

  rstd   `1.0f / sqrtf((float)var + eps)`: the cast and the add put 2u on var + eps, the root halves that, root and divide add u each:  g_3.
  scale  `ga * rstd`:  g_4.
  shift  `be - (float)mean * ga * rstd`: the product is mean(1+u) * ga (1+u) * rstd(1+3u) (1+u) = g_6 |mean sc|, the subtract u (|be| + |mean sc|).
  y      `o = x * sc + sh; o += res; relu; store`: x sc carries g_5, the first add u (|x sc| + |sh|), the second u (|x sc| + |sh| + |res|), so
           E = g_7 |x sc| + g_9 |mean sc| + g_3 |beta| + g_1 |res|            (the proposed 8u is one short on the mean term, one over on x sc)
           |y - y64| <= E + bT (|y64| + E).        fmaxf adds nothing.  bT is the proposed b, on the computed value (y64 off by at most E) instead of on y64.
         With res_scale_shift the residual is r = round_T(res_in * rsc + rsh), a ReLU-free BatchNorm output with no residual of its own:
           E_r = g_6 |x sc| + g_8 |mean sc| + g_2 |beta|,  |r - r64| <= R = E_r + bT (|r64| + E_r);  y's E takes |res| = |r64| + R and adds R.
  mask   an element with |pre-activation64| <= E is ambiguous: left out of dres / dx, its |dy xhat| added to the dgamma bound, its |dy| / V to c1's.
  s2     `s2 += gv * (xv - mu) * rs` (bn_partial_kernel MODE 1, bn_small_bwd_kernel): mu = fl32(mean) is off by u |mean| ABSOLUTELY, which no
         multiple of |g xhat| covers when x is near the mean, so that term is separate: u |g| |mean| rstd.  Relative to |g xhat|: subtract u,
         two products 2u, rs 3u = g_6; at most n32 - 1 fp32 additions of non-zero terms meet before the first conversion to double (adding an
         exact zero rounds nothing), n32 = rows_per_chunk for the three-kernel form and V for the one-launch form; one or two casts of the sum:
           E_s2[b, c] = g_(n32+8) sum |g xhat| + u |mean| rstd sum |g|  (+ the ambiguous terms);  dgamma: sum over b (+ u |result| with accumulate).
  dx     `sc * (g - c1 - xh * c2)`: c1 = fl32(s1 / V) u; xh = (x - mu) * rs: g_5 |xhat| + u |mean| rstd; xh c2: + u and |xhat| dc2 with
         dc2 = E_s2 / V; two subtracts u each on at most |g| + |c1| + |xhat c2|; sc g_4 and the product u:
           E_dx = |sc| (g_8 |g| + g_8 |c1| + g_12 |xhat c2| + |xhat| dc2 + u |mean| rstd |c2| + dc1),   |dx - dx64| <= E_dx + bT (|dx64| + E_dx).
  running statistics  `rm = (1.f - m) * rm + m * mean` per grid: (1 - m) u, its product u, mean's cast and product 2u on a tenth, the add u:
         <= 3.1u max(|rm|, |mean|) per grid, earlier errors shrink by 0.9: (3B + 2) u max(|initial|, |per-grid value|) for B <= 20.  The
         variance takes one or two casts on the way to `unbiased` (three-kernel / one-launch), still within 3.1u per grid.
"""
import dataclasses
import functools
import zlib

import numpy as np
import torch

U = 2.0 ** -24
BFU = 2.0 ** -8
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))
LIMIT = 2 ** 24
F64 = torch.float64
AMBIGUOUS_CAP = 1e-4
BNS_ROWS, BNS_COLS = 64, 4


def g_(n):
    return n * U / (1 - n * U)


def rows_per_chunk(V):
    """bn_rows_per_chunk of csrc/fpn_ops.hip (tests/test_bn_host.py holds it to dreg_bn_num_chunks)"""
    return 512 if V >= 262144 else 256 if V >= 32768 else 128 if V >= 4096 else 32 if V >= 512 else (8 if V >= 8 else V)


def colsum_rows_per_chunk(M):
    r = (M + 255) // 256
    return max(32, (r + 31) // 32 * 32)


def small_ok(B, V, C, dt):
    return 2 <= V <= 512 and C % (BNS_COLS * (8 if dt == 0 else 4)) == 0 and B >= 1


def path_of(B, V, C, dt):
    """the launch form a training-mode [B, V, C] layer takes at default knobs: bn3d_fwd_impl / bn3d_bwd_impl"""
    if not small_ok(B, V, C, dt):
        return "three"
    return "nr8" if V == 8 * BNS_ROWS else "nr1" if V == BNS_ROWS else "nr0"


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    B: int
    V: int
    C: int
    dt: int                     # 0 bf16, 1 fp32
    path: str                   # "three" | "nr0" | "nr1" | "nr8": the launch form the case must reach
    res: bool = True
    relu: bool = True
    form: str = "plain"         # plain | ynull | acc | eval | from_sums | res_ss | splitk | defer
    rpc: int = 0                # from_sums: rows per chunk of the sums the test forms
    const: tuple = ()           # channels held constant (var = 0, rstd = 1 / sqrt(eps))
    reaches: str = ""

    @property
    def id(self):
        return self.name.replace(" ", "_")

    @property
    def n32(self):
        return rows_per_chunk(self.V) if self.path == "three" else self.V


def _both(name, B, V, C, path, **kw):
    return [Case(f"{name} {'bf16' if dt == 0 else 'fp32'}", B, V, C, dt, path, **kw) for dt in (0, 1)]


def _combos(name, B, V, C, dt, path, **kw):
    return [Case(f"{name} res{int(r)} relu{int(l)}", B, V, C, dt, path, res=r, relu=l, **kw) for r in (True, False) for l in (True, False)]


# ---- three-kernel form: bn_partial / bn_finalize / bn_apply_cols (and their backward siblings)
THREE = (
    _combos("three 2x210x24 bf16", 2, 210, 24, 0, "three", reaches="rpc 8, 27 chunks, 2-row tail, rpi 85 > rpc, idle last thread")
    + _combos("three 2x210x24 fp32", 2, 210, 24, 1, "three", reaches="rpc 8, 27 chunks, 2-row tail, rpi 42 > rpc, idle last threads")
    + _both("three 3x4099x64", 3, 4099, 64, "three", reaches="rpc 128, 3-row tail, u-unroll tail")
    + _both("three 1x513x32", 1, 513, 32, "three", reaches="first V past the small form")
    + _both("three 9x8320x16", 9, 8320, 16, "three", reaches="65 chunks (lane loop wraps), 9 grids (wave loop wraps)")
    + [Case("three 1x600x2048 fp32 two slabs", 1, 600, 2048, 1, "three", reaches="blockIdx.z = 1"),
       Case("three 1x600x4096 bf16 two slabs", 1, 600, 4096, 0, "three", reaches="blockIdx.z = 1 in bf16"),
       Case("three 1x32773x8 bf16", 1, 32773, 8, 0, "three", reaches="rpc 256"),
       Case("three 1x262149x8 bf16", 1, 262149, 8, 0, "three", reaches="rpc 512")]
    + [Case("three 2x210x24 bf16 ynull", 2, 210, 24, 0, "three", res=False, form="ynull"),
       Case("three 3x4099x64 fp32 ynull", 3, 4099, 64, 1, "three", res=False, form="ynull"),
       Case("three 2x210x24 bf16 accumulate", 2, 210, 24, 0, "three", form="acc"),
       Case("three 9x8320x16 fp32 accumulate", 9, 8320, 16, 1, "three", res=False, form="acc")]
)
# ---- one-launch form: bn_small_fwd_kernel / bn_small_bwd_kernel <NR = 0, 1, 8>
_SMALL_SHAPES = ((2, 32, 16, "nr0", "smallest V, a constant channel"), (210, 64, 64, "nr0", "NR 0, ragged by 64"),
                 (64, 32, 32, "nr1", "NR 1"), (512, 32, 32, "nr8", "NR 8"))          # (V, C bf16, C fp32, path, what it reaches)
SMALL = (
    [Case(f"small 1x{V}x{(Cb, Cf)[dt]} {('bf16', 'fp32')[dt]}", 1, V, (Cb, Cf)[dt], dt, p, const=(3,) if V == 2 else (), reaches=why)
     for V, Cb, Cf, p, why in _SMALL_SHAPES for dt in (0, 1)]
    + [Case("small 3x2x32 bf16", 3, 2, 32, 0, "nr0", const=(5,)), Case("small 3x2x16 fp32", 3, 2, 16, 1, "nr0", const=(3,))]
    + [c for V, Cb, Cf, p, _ in _SMALL_SHAPES[1:] for dt in (0, 1) for c in _combos(f"small 3x{V}x{Cb} {('bf16', 'fp32')[dt]}", 3, V, Cb, dt, p)]
    + [c for V, Cb, Cf, p, _ in _SMALL_SHAPES[1:] for c in _both(f"small 3x{V}x{Cb} ynull", 3, V, Cb, p, res=False, form="ynull")]
    + [Case("small 3x512x32 bf16 accumulate", 3, 512, 32, 0, "nr8", form="acc"),
       Case("small 3x210x64 fp32 accumulate", 3, 210, 64, 1, "nr0", form="acc")]
)
TRAIN = THREE + SMALL
EVAL = _both("eval 2x210x24", 2, 210, 24, "three", form="eval") + _both("eval 2x64x32", 2, 64, 32, "three", form="eval", relu=False)
FROM_SUMS = (_both("from_sums 2x8320x16 rpc 128", 2, 8320, 16, "three", form="from_sums", rpc=128)
             + _both("from_sums 2x8320x16 one chunk", 2, 8320, 16, "three", form="from_sums", rpc=8320)
             + [Case("from_sums 2x64x32 bf16 small shape", 2, 64, 32, 0, "three", form="from_sums", rpc=32)])
RES_SS = _both("res_ss 2x210x24", 2, 210, 24, "three", form="res_ss") + _both("res_ss 3x4099x64", 3, 4099, 64, "three", form="res_ss")
SPLITK = ([Case(f"splitk 3x{V}x32 {'bf16' if dt == 0 else 'fp32'}", 3, V, 32, dt, "nr1" if V == 64 else "nr8", form="splitk")
           for V in (64, 512) for dt in (0, 1)])
DEFER = [[Case(f"defer 3x{V}x{C} {'bf16' if dt == 0 else 'fp32'}", 3, V, C, dt, p, form="defer") for V, C, p in ((512, 32, "nr8"), (210, 288, "nr0"), (64, 512, "nr1"))]
         for dt in (0, 1)]
ALL = TRAIN + EVAL + FROM_SUMS + RES_SS + SPLITK + [c for grp in DEFER for c in grp]

# contracts that must come back as DREG_EINVAL without a launch: (name, entry, B, V, C, dt, what)
EINVAL = [
    ("split-K outside the register-resident form, fwd", "fwd_splitk", 2, 210, 64, 0),
    ("split-K outside the register-resident form, bwd", "bwd_splitk", 2, 210, 64, 0),
    ("split-K on the three-kernel form, fwd", "fwd_splitk", 2, 513, 32, 0),
    ("res_scale_shift on the small path", "fwd_res_ss", 2, 64, 32, 0),
    ("y == NULL on the small path", "fwd_ynull", 2, 64, 32, 0),
    ("train with V < 2", "fwd", 2, 1, 32, 0),
    ("B > 256, fwd", "fwd", 257, 2, 8, 0),
    ("B > 256, bwd", "bwd", 257, 2, 8, 0),
    ("C % G != 0 bf16, fwd", "fwd", 2, 210, 20, 0),
    ("C % G != 0 fp32, bwd", "bwd", 2, 210, 18, 1),
    ("ragged last slab fp32 C 1536, fwd", "fwd", 1, 600, 1536, 1),
    ("ragged last slab fp32 C 1536, bwd", "bwd", 1, 600, 1536, 1),
    ("ragged last slab bf16 C 2056, fwd", "fwd", 1, 600, 2056, 0),
    ("ragged last slab fp32 C 1536, colsum", "colsum", 1, 600, 1536, 1),
    ("ragged last slab fp32 C 1536, colsum_rows", "colsum_rows", 1, 600, 1536, 1),
    ("ragged last slab C 2056, fused stem forward", "stem_fwd", 1, 512, 2056, 0),
]

COLSUM = [(M, C, dt) for M in (1, 31, 33, 8191, 8193) for C, dt in ((8, 0), (24, 0), (2048, 0), (2048, 1))]
COLSUM_ROWS = [(1, 24, 0), (77, 24, 0), (1, 2048, 1), (77, 2048, 1)]          # (rows in the list, C, dtype) of a [500, C] tensor
COLSUM_BATCHED = [(33, 8, 0), (8193, 24, 1), (1000, 2048, 0)]                 # (M, C, accumulate) of one batched launch (bf16)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


@functools.lru_cache(maxsize=3)
def operands(c):
    """x, dy, res [B, V, C] and the per-channel tensors, all fp64 holding values the case's dtype (and fp32 for the parameters) represents"""
    r = _rng(c.name)
    B, V, C = c.B, c.V, c.C
    off = r.randint(-4, 5, size=C)
    x = r.randint(-7, 9, size=(B, V, C)) + off
    for ch in c.const:
        x[:, :, ch] = off[ch] + 5
    dy = r.randint(-7, 9, size=(B, V, C))
    res = r.randint(-8, 9, size=(B, V, C)) / 4.0
    gamma = (1 + 0.1 * r.randn(C)).astype(np.float32)
    beta = (0.1 * r.randn(C)).astype(np.float32)
    for ch in c.const:
        beta[ch] = np.float32(0.0625 if beta[ch] >= 0 else -0.0625)
    o = dict(x=_t(x), dy=_t(dy), res=_t(res), gamma=_t(gamma), beta=_t(beta),
             rm0=_t((0.1 * r.randn(C)).astype(np.float32)), rv0=_t((1 + 0.1 * r.rand(C)).astype(np.float32)),
             dgamma0=_t(r.randn(C).astype(np.float32)), dbeta0=_t(r.randint(-50, 51, size=C)))
    if c.form == "res_ss":      # the unapplied BatchNorm whose input is the residual: its own parameters
        o.update(gamma_r=_t((1 + 0.1 * r.randn(C)).astype(np.float32)), beta_r=_t((0.1 * r.randn(C)).astype(np.float32)),
                 xr=_t(r.randint(-7, 9, size=(B, V, C)) + r.randint(-4, 5, size=C)))
    if c.form == "splitk":      # three fp32 slices each: x's sum to x, dy's to integers up to 300 in size (a bf16 dy has to round them)
        big = r.randint(-300, 301, size=(B, V, C))
        for key, total in (("x", x), ("dy", big)):
            s0, s1 = r.randint(-40, 41, size=(B, V, C)), r.randint(-40, 41, size=(B, V, C))
            o[key + "_slices"] = _t(np.stack([s0, s1, total - s0 - s1]))
        o["dy"] = rounded(_t(big), c.dt)
    return o


def rounded(t, dt):
    """what a store of the case's dtype leaves (round to nearest even), back in fp64"""
    return t.float().to(torch.bfloat16 if dt == 0 else torch.float32).double()


# ------------------------------------------------------------------------------------------------ the fp64 reference and its bounds
def stats(x, V):
    """per-grid (mean, biased variance), evaluated as the kernels do in double: exact sums, one division, one product, one subtract"""
    s1, s2 = x.sum(1), (x * x).sum(1)
    mean = s1 / V
    var = (s2 / V - mean * mean).clamp_(min=0)
    return mean, var


def forward(c, x, gamma, beta, res=None, res_err=None, mean=None, var=None):
    """y64 and the bounds.  res_err: the bound R on |res_kernel - res| when the residual is itself computed (res_scale_shift).
    mean / var given: eval mode (per-channel running statistics instead of the grid's own)."""
    bT = BFU if c.dt == 0 else 0.0
    if mean is None:
        mean, var = stats(x, c.V)
    else:
        mean, var = mean.expand(c.B, -1), var.expand(c.B, -1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    sc = gamma * rstd
    msc = mean * sc
    xsc = x * sc[:, None]
    pre = (x - mean[:, None]) * sc[:, None] + beta
    E = g_(7) * xsc.abs() + (g_(9) * msc.abs() + g_(3) * beta.abs())[:, None]
    if res is not None:
        pre = pre + res
        E = E + g_(1) * res.abs()
        if res_err is not None:
            E = E + (1 + g_(1)) * res_err
    y = pre.clamp(min=0) if c.relu else pre
    return dict(mean=mean, var=var, rstd=rstd, sc=sc, sh=beta - msc, pre=pre, y=y, E=E, y_tol=E + bT * (y.abs() + E),
                rstd_tol=g_(3) * rstd, sc_tol=g_(4) * sc.abs(), sh_tol=g_(7) * msc.abs() + U * beta.abs(),
                amb=(pre.abs() <= E) if c.relu else torch.zeros_like(pre, dtype=torch.bool))


def unapplied_residual(c, xr, gamma_r, beta_r):
    """the output of a ReLU-free, residual-free BatchNorm formed on the fly from its input and (scale, shift): value and bound R"""
    bT = BFU if c.dt == 0 else 0.0
    mean, var = stats(xr, c.V)
    rstd = 1.0 / torch.sqrt(var + EPS)
    sc = gamma_r * rstd
    r64 = (xr - mean[:, None]) * sc[:, None] + beta_r
    Er = g_(6) * (xr * sc[:, None]).abs() + (g_(8) * (mean * sc).abs() + g_(2) * beta_r.abs())[:, None]
    return r64, Er + bT * (r64.abs() + Er)


def running(c, f, rm0, rv0):
    """sequential over the grids, as one BatchNorm call per grid; (value, tolerance) for the mean and the variance"""
    rm, rv = rm0.clone(), rv0.clone()
    unb = f["var"] * c.V / (c.V - 1)
    for b in range(c.B):
        rm = (1 - MOM) * rm + MOM * f["mean"][b]
        rv = (1 - MOM) * rv + MOM * unb[b]
    k = (3 * c.B + 2) * U
    return rm, k * torch.maximum(rm0.abs(), f["mean"].abs().amax(0)), rv, k * torch.maximum(rv0.abs(), unb.abs().amax(0))


def backward(c, x, dy, f, accumulate=False, dgamma0=None, dbeta0=None):
    bT = BFU if c.dt == 0 else 0.0
    V = c.V
    amb = f["amb"]
    g = dy * (f["pre"] > 0) if c.relu else dy
    mean, rstd, sc = f["mean"], f["rstd"], f["sc"]
    xhat = (x - mean[:, None]) * rstd[:, None]
    s1, s2 = g.sum(1), (g * xhat).sum(1)
    amb_s1 = (amb * dy.abs()).sum(1)
    E_s2 = g_(c.n32 + 8) * (g * xhat).abs().sum(1) + U * mean.abs() * rstd * g.abs().sum(1) + (amb * (dy * xhat).abs()).sum(1)
    c1, c2 = s1 / V, s2 / V
    dx = sc[:, None] * (g - c1[:, None] - xhat * c2[:, None])
    E_dx = sc.abs()[:, None] * (g_(8) * g.abs() + (g_(8) * c1.abs() + amb_s1 / V)[:, None] + g_(12) * (xhat * c2[:, None]).abs()
                                + xhat.abs() * (E_s2 / V)[:, None] + (U * mean.abs() * rstd * c2.abs())[:, None])
    dgamma, dbeta, E_dg = s2.sum(0), s1.sum(0), E_s2.sum(0)
    if accumulate:
        dgamma, dbeta = dgamma + dgamma0, dbeta + dbeta0
        E_dg = E_dg + U * dgamma.abs()
    return dict(g=g, dx=dx, dx_tol=E_dx + bT * (dx.abs() + E_dx), dgamma=dgamma, dgamma_tol=E_dg, dbeta=dbeta, dbeta_exact=amb_s1.sum(0) == 0,
                s1=s1, s2=s2, s2_tol=E_s2, keep=~amb)


def chunk_sums(x, rpc):
    """[B][V / rpc][C][2] = (sum x, sum x^2) per chunk: what dreg_conv3d_igemm_bnstats leaves for dreg_bn3d_fwd_from_sums"""
    B, V, C = x.shape
    xc = x.reshape(B, V // rpc, rpc, C)
    return torch.stack([xc.sum(2), (xc * xc).sum(2)], dim=-1)


def worst_partial(c, x=None):
    """the largest fp32 partial sum a kernel forms before it continues in double: per chunk of the three-kernel form, per grid of the other"""
    x = operands(c)["x"] if x is None else x
    n = c.rpc if c.form == "from_sums" else c.n32
    pad = (-c.V) % n
    xx = torch.nn.functional.pad(x * x, (0, 0, 0, pad)).reshape(c.B, -1, n, c.C)
    return float(xx.sum(2).max())


def reference(c):
    """the forward reference of a case from its own operands (the GPU test and the host test share it)"""
    o = operands(c)
    if c.form == "eval":
        return forward(c, o["x"], o["gamma"], o["beta"], o["res"] if c.res else None, mean=o["rm0"][None], var=o["rv0"][None])
    if c.form == "res_ss":
        r64, R = unapplied_residual(c, o["xr"], o["gamma_r"], o["beta_r"])
        return forward(c, o["x"], o["gamma"], o["beta"], r64, res_err=R)
    return forward(c, o["x"], o["gamma"], o["beta"], o["res"] if c.res else None)


def colsum_operand(M, C, name):
    r = _rng(f"colsum {name} {M} {C}")
    return _t(r.randint(-8, 9, size=(M, C))), _t(r.randint(-100, 101, size=C))


# ------------------------------------------------------------------------------------------------ the C ABI pieces both test files use
import ctypes  # noqa: E402


class BnExtra(ctypes.Structure):
    """dreg_bn_extra of include/dreg_nerf.h"""
    _fields_ = [("res_scale_shift", ctypes.c_void_p), ("splitk_part", ctypes.c_void_p), ("splitk_nsplit", ctypes.c_int), ("splitk_slice", ctypes.c_size_t)]


def refused_call(lib, entry, B, V, C, dt, p, stream):
    """one call of the EINVAL table; p(name) -> pointer (None where the host test has no buffer; `part` / `ss2` must be non-null addresses)"""
    fwd = (p("x"), p("res"), p("y"), p("gamma"), p("beta"), p("rm"), p("rv"), p("ss"), p("mr"), p("ws"), B, V, C, EPS, MOM, 1, 1, dt)
    bwd = (p("x"), p("dy"), p("y"), p("ss"), p("mr"), p("dx"), p("dres"), p("dgamma"), p("dbeta"), p("coef"), p("ws"), B, V, C, 1, 0, dt)
    if entry == "fwd":
        return lib.dreg_bn3d_fwd(*fwd, stream)
    if entry == "bwd":
        return lib.dreg_bn3d_bwd(*bwd, stream)
    if entry == "fwd_ynull":
        return lib.dreg_bn3d_fwd_ex(p("x"), None, None, *fwd[3:], None, None, 0, None, stream)
    if entry == "fwd_res_ss":
        ex = BnExtra(p("ss2"), None, 0, 0)
        return lib.dreg_bn3d_fwd_ex(*fwd, None, None, 0, ctypes.addressof(ex), stream)
    ex = BnExtra(None, p("part"), 3, B * V * C)
    if entry == "fwd_splitk":
        return lib.dreg_bn3d_fwd_ex(*fwd, None, None, 0, ctypes.addressof(ex), stream)
    if entry == "bwd_splitk":
        return lib.dreg_bn3d_bwd_ex(*bwd, None, None, ctypes.addressof(ex), stream)
    if entry == "colsum":
        return lib.dreg_colsum(p("x"), p("dgamma"), p("ws"), V, C, 0, dt, stream)
    if entry == "colsum_rows":
        return lib.dreg_colsum_rows(p("x"), p("rows"), V, p("dgamma"), p("ws"), C, 0, dt, stream)
    if entry == "stem_fwd":
        assert V == 512
        return lib.dreg_bn_relu_maxpool_fwd(p("x"), p("y"), p("argmax"), *fwd[3:10], B, 8, 8, 8, 4, 4, 4, C, EPS, MOM, 1, 1, stream)
    raise AssertionError(entry)
