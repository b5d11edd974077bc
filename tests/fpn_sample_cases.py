"""Cases for the pooling and trilinear-gather kernels of csrc/fpn_ops.hip: tests/test_fpn_sample_host.py (no GPU) and
tests/test_hip_fpn_sample_fp64.py (GPU) share the seeded operands, the fp64 references, the bounds and the case tables below.  Imports
without a GPU.  U, BFU, g_(n) and `rounded` are tests/bn_cases.py's; the library is built with -ffp-contract=off, so ONE fp32 expression
written element-wise in numpy / torch float32 gives the kernel's bits.  That is used for SELECTORS only (arg-max taps, the ReLU mask, the
trilinear coordinate weights): no element is "ambiguous".  Values are compared in fp64.

Two regimes.
  EXACT (torch.equal).  Max-pool and downsample-sum on small integers; the trilinear forms on geometries whose per-axis step
      s = (n_in - 1) / (n_out - 1) is dyadic (every f = i s is exact in fp32, every weight a multiple of 1/64) with integer features and
      gradients in [-8, 8]: every product and partial sum is a multiple of a fixed quantum q (1/64; 1/512 for the segment forms, whose 1/cnt is
      a power of two) and stays below 2^24 q, so it is exact in fp32 in ANY order, atomics included.  Outputs equal round_T(fp64 value).
  COUNTED (|got - fp64| <= bound).  Terms are t_c = w_c v_c with w_c the restated fp32 corner weight and v_c the operand, all in fp64.
      forward   `acc += v[k] * wgt` over the 8 corners from acc = 0: one product and seven additions (0 + x is exact): g_(8) sum|t_c|,
                + BFU |out64| for a bf16 store.
      segment   gather_segment_mean_kernel `acc += smp` over cnt members from 0, `inv = 1.f / cnt`, `acc * inv`:
                g_(8 + cnt - 1 + 2) sum over members sum|t_c|.
      backward  K = number of corner terms with w != 0 that reach a coarse element: `g * wgt` one product, K - 1 additions onto 0; the issue
                allows g_(K + 1) sum|w g|, + BFU |dp64| for a bf16 store, + one rounding per term for the SEG product `r * ss`.  The atomic and
                the gather forms share it, with one addition for the gather form, from tri_weight(): where an axis is clamped (i0 == i1 == n_in - 1)
                with t != 0 (f = fl(i s) landed above n_in - 1 for the last fine voxel) the gather kernel weights the point ONCE by
                fl((1 - t) + t) per such axis (<= 3 roundings) times the other axes (`(wz * wx) * wy`: 2 roundings), where the reference sums
                the corner terms whose restated weights carry 2 roundings each: <= 7 roundings on those terms, g_(7) sum over them |w g|.
  Fused stem: step 1 holds mean_rstd / scale_shift / running statistics to bn_cases.forward / running (the three-kernel bounds, imported);
      step 2 takes the DEVICE's scale_shift and restates o = round_bf16(max(fl32(fl32(x sc) + sh), 0)) and the first-maximum pool of o: pooled
      values and arg-max bytes torch.equal.  Backward: dy64 = dp un-pooled through the (checked) taps, masked by the restated x sc + sh > 0,
      then bn_cases.backward with relu off (the mask is already applied, no element ambiguous) and n32 = rows_per_chunk(V).
      bn_pool_bwd_kernel MODE 0 reading: a thread sums `s2[k] += g[k] * xh` over its ceil(rpc / rpi) rows, then `a2[i] += red[..]` adds rpi
      values from LDS starting at 0; one column of a chunk is a sum of at most rpc non-zero terms in some order, so at most rpc - 1 additions
      round (adding an exact zero rounds nothing): the same n32 - 1 as bn_partial_kernel; `xh = (xv - mu) * rs`, `g * xh` are its g_6; the sums
      continue in bn_bwd_finalize_kernel exactly as the three-kernel form's.  The un-pooled gradient (<= 8 integers) is exact and never rounded
      to bf16.  The count is bn_cases.backward's, unchanged.  No constant here was fitted to a GPU result.

Max-pool reference: F.max_pool3d(return_indices=True) in fp64 on the CPU; its first-maximum rule in z, y, x scan order equals the kernel's
strict `>` (the host test holds it to a brute-force numpy argmax over the 27 taps, which returns the first maximum by definition).
A window that holds one voxel (extent-1 volume) cannot tie; the tie share is taken over the windows with two voxels or more.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

import bn_cases as N
from bn_cases import BFU, U, g_, rounded  # noqa: F401  (re-exported for the two test files)

F64 = torch.float64
f32 = np.float32
LIMIT = 2 ** 24


def _rng(name):
    return N._rng("fpn sample " + name)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def G_of(dt):
    return 8 if dt == 0 else 4


def dt_name(dt):
    return "bf16" if dt == 0 else "fp32"


# ================================================================================================ 1. max-pool 3^3 s2 p1
def pooled_extent(n):
    return (n - 1) // 2 + 1


@dataclasses.dataclass(frozen=True)
class PoolCase:
    B: int
    D: int
    H: int
    W: int
    C: int
    dt: int
    lo: int = -3                # x is drawn from the integers [lo, 3]: a narrower range where the windows are small, so that they still tie
    reaches: str = ""

    @property
    def name(self):
        return f"pool {self.B}x{self.D}x{self.H}x{self.W}x{self.C} {dt_name(self.dt)}"

    @property
    def id(self):
        return self.name.replace(" ", "_")

    @property
    def out(self):
        return pooled_extent(self.D), pooled_extent(self.H), pooled_extent(self.W)


POOL = [
    PoolCase(1, 1, 1, 1, 8, 0, reaches="every extent 1: one window of one voxel, C = G"),
    PoolCase(2, 1, 2, 5, 8, 0, lo=1, reaches="extents 1 and 2, odd W"),
    PoolCase(2, 4, 7, 6, 24, 0, reaches="odd and even extents, CG = 3"),
    PoolCase(1, 9, 8, 7, 40, 0, reaches="CG = 5"),
    PoolCase(3, 6, 6, 6, 64, 0, reaches="C = 64, three grids"),
    PoolCase(1, 1, 1, 1, 4, 1, reaches="every extent 1, fp32, C = G"),
    PoolCase(2, 1, 2, 5, 4, 1, lo=1, reaches="extents 1 and 2, fp32"),
    PoolCase(2, 4, 7, 6, 12, 1, reaches="fp32 CG = 3"),
    PoolCase(1, 9, 8, 7, 12, 1, reaches="fp32 odd extents"),
    PoolCase(3, 6, 6, 6, 64, 1, reaches="fp32 C = 64"),
]


@functools.lru_cache(maxsize=None)
def pool_operands(c):
    r = _rng(c.name)
    Do, Ho, Wo = c.out
    return dict(x=_t(r.randint(c.lo, 4, size=(c.B, c.D, c.H, c.W, c.C))), dy=_t(r.randint(-7, 9, size=(c.B, Do, Ho, Wo, c.C))),
                dx0=_t(r.randint(-7, 9, size=(c.B, c.D, c.H, c.W, c.C))))


def pool_forward(x):
    """x [B, D, H, W, C] fp64 -> (pooled [B, Do, Ho, Wo, C] fp64, tap codes (dz*3+dy)*3+dx as uint8, flat input index int64 [B, C, Do, Ho, Wo])"""
    B, D, H, W, C = x.shape
    y, idx = F.max_pool3d(x.permute(0, 4, 1, 2, 3).contiguous(), 3, 2, 1, return_indices=True)
    Do, Ho, Wo = y.shape[2:]
    iz, iy, ix = idx // (H * W), (idx // W) % H, idx % W
    oz = torch.arange(Do).view(1, 1, Do, 1, 1)
    oy = torch.arange(Ho).view(1, 1, 1, Ho, 1)
    ox = torch.arange(Wo).view(1, 1, 1, 1, Wo)
    tap = ((iz - (2 * oz - 1)) * 3 + (iy - (2 * oy - 1))) * 3 + (ix - (2 * ox - 1))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 26
    return y.permute(0, 2, 3, 4, 1).contiguous(), tap.permute(0, 2, 3, 4, 1).contiguous().to(torch.uint8), idx


def pool_backward(dy, idx, D, H, W):
    """dy [B, Do, Ho, Wo, C] fp64 scattered through the flat arg-max indices: dx [B, D, H, W, C]"""
    B, C = idx.shape[:2]
    dx = torch.zeros(B, C, D * H * W, dtype=F64)
    dx.scatter_add_(2, idx.reshape(B, C, -1), dy.permute(0, 4, 1, 2, 3).reshape(B, C, -1))
    return dx.reshape(B, C, D, H, W).permute(0, 2, 3, 4, 1).contiguous()


def pool_windows(x):
    """[B, Do, Ho, Wo, C, 27] fp64: the window of every pooled element in tap order, -inf where the tap is outside the volume"""
    xp = F.pad(x.permute(0, 4, 1, 2, 3), (1, 1, 1, 1, 1, 1), value=float("-inf"))
    w = xp.unfold(2, 3, 2).unfold(3, 3, 2).unfold(4, 3, 2)                 # [B, C, Do, Ho, Wo, 3, 3, 3]
    return w.reshape(*w.shape[:5], 27).permute(0, 2, 3, 4, 1, 5).contiguous()


# ================================================================================================ 2. fused stem (bf16)
@dataclasses.dataclass(frozen=True)
class StemCase:
    B: int
    D: int
    H: int
    W: int
    C: int
    reaches: str = ""

    @property
    def name(self):
        return f"stem {self.B}x{self.D}x{self.H}x{self.W}x{self.C}"

    @property
    def id(self):
        return self.name.replace(" ", "_")

    @property
    def V(self):
        return self.D * self.H * self.W

    @property
    def out(self):
        return pooled_extent(self.D), pooled_extent(self.H), pooled_extent(self.W)

    def bn(self, relu=True):
        """the bn_cases.Case whose operands, reference and bounds this case uses: [B, V, C] bf16, three-kernel form"""
        return N.Case(self.name, self.B, self.V, self.C, 0, "three", res=False, relu=relu)


def slabs_ragged(CG):
    """slabs_ragged of csrc/fpn_ops.hip"""
    return CG > 256 and CG % 256 != 0


# C = 2056 (CG = 257) is what one would want for "the second slab", but slabs_ragged refuses it (the EINVAL table below has it);
# the smallest admitted C above 2048 is 4096 (CG = 512, two full slabs).
STEM = [
    StemCase(2, 12, 10, 14, 64, reaches="rpc 32, 53 chunks, rpi 32"),
    StemCase(1, 9, 11, 7, 16, reaches="odd extents, rpi 128 > rpc 32"),
    StemCase(3, 2, 2, 2, 8, reaches="V = 8: one chunk, one pooled voxel, rpi 256"),
    StemCase(1, 2, 3, 2, 4096, reaches="two channel slabs (blockIdx.z = 1)"),
]


@functools.lru_cache(maxsize=2)
def stem_operands(c):
    o = dict(N.operands(c.bn()))
    Do, Ho, Wo = c.out
    o["dp"] = _t(_rng(c.name + " dp").randint(-7, 9, size=(c.B, Do, Ho, Wo, c.C)))
    return o


def stem_activation(x, ss, relu):
    """o = round_bf16([max](fl32(fl32(x sc) + sh), 0)) with the device's fp32 scale_shift [B, C, 2]: the kernel's expression, bit for bit.
    x [B, D, H, W, C] fp64 (bf16 values).  Returns (o as fp64, the fp32 pre-activation)"""
    B, C = ss.shape[:2]
    sc, sh = ss[..., 0].float().view(B, 1, 1, 1, C), ss[..., 1].float().view(B, 1, 1, 1, C)
    pre = x.float() * sc
    pre = pre + sh
    o = torch.clamp(pre, min=0) if relu else pre
    return o.to(torch.bfloat16).double(), pre


# ================================================================================================ 3. 2x downsample-sum
@dataclasses.dataclass(frozen=True)
class DownCase:
    coarse: tuple
    fine: tuple                 # each extent 2 n or 2 n - 1 of its coarse one (the cropped child)
    C: int
    dt: int
    B: int = 2

    @property
    def name(self):
        return f"down {'x'.join(map(str, self.coarse))} from {'x'.join(map(str, self.fine))} C{self.C} {dt_name(self.dt)}"

    @property
    def id(self):
        return self.name.replace(" ", "_")


DOWN = [DownCase(co, fi, C, dt) for co, fi in (((3, 2, 4), (6, 3, 8)), ((3, 2, 4), (5, 4, 7)), ((1, 5, 2), (1, 9, 4)), ((2, 1, 3), (4, 2, 5)))
        for C, dt in ((8, 0), (24, 0), (4, 1), (12, 1))]
DOWN_SENTINEL = 77.0
ROW_LISTS = ("random", "one", "full", "empty")


@functools.lru_cache(maxsize=None)
def down_operands(c):
    return _t(_rng(c.name).randint(-8, 9, size=(c.B, *c.fine, c.C)))


def down_reference(c, g):
    out = torch.zeros(c.B, *c.coarse, c.C, dtype=F64)
    Df, Hf, Wf = c.fine
    for a in range(2):
        for b in range(2):
            for d in range(2):
                ch = g[:, a::2, b::2, d::2]
                out[:, :ch.shape[1], :ch.shape[2], :ch.shape[3]] += ch
    return out


def down_rows(c, kind):
    n = c.B * c.coarse[0] * c.coarse[1] * c.coarse[2]
    r = _rng(c.name + " rows " + kind)
    if kind == "random":
        return np.sort(r.choice(n, size=max(1, int(round(0.3 * n))), replace=False)).astype(np.int32)
    return {"one": np.array([r.randint(n)], np.int32), "full": np.arange(n, dtype=np.int32), "empty": np.zeros(0, np.int32)}[kind]


# ================================================================================================ 4. trilinear gather
def tri_axis(n_out, n_in):
    """tri_axis of csrc/fpn_ops.hip for every fine coordinate of one axis, in numpy float32: (i0, i1, t, f)"""
    i = np.arange(n_out, dtype=f32)
    s = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    f = (i * s).astype(f32)
    i0 = np.minimum(f.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    t = (f - i0.astype(f32)).astype(f32)
    return i0, i1, t, f


def axis_bound(n_in):
    """|restated fp32 per-axis weight - exact rational align-corners weight| (host test)"""
    return (2 * (n_in - 1) + 3) * U


EXACT_PAIRS = ((9, 5), (17, 5), (5, 5), (5, 9), (9, 3), (13, 4), (13, 7), (7, 13), (2, 2), (1, 3), (4, 1))
GENERAL_PAIRS = ((10, 5), (12, 6), (14, 7), (11, 4), (6, 11), (33, 17))
SWEEP_BIG = ((128, 64), (127, 64), (128, 63), (100, 99), (99, 100), (200, 3), (3, 200), (257, 256))
SWEEP = ([(0, no, ni) for ni in range(1, 11) for no in range(1, 21)] + [(ax, no, ni) for ax in range(3) for no, ni in SWEEP_BIG])   # (axis, n_out, n_in)

FWD_FORMS = ("fwd bf16->fp32", "fwd bf16->bf16", "fwd fp32->fp32", "segmean bf16", "segmean fp32")
INSTANTIATIONS = (set(FWD_FORMS) | {"bwd atomic fp32", "bwd_rows bf16", "bwd_rows fp32"}
                  | {f"{k} {dt_name(dt)} CPL{cpl}" for k in ("gather", "gather_seg") for dt in (0, 1) for cpl in (1, 2, 3, 4)})


@dataclasses.dataclass(frozen=True)
class TriCase:
    label: str
    z: tuple                    # (n_out, n_in) = (Zr, d)
    x: tuple                    # (Xr, h)
    y: tuple                    # (Yr, w)
    C: int
    exact: bool
    B: int = 3                  # grid 1 holds no point
    seg: bool = False           # B = 4: two pairs over four grids, points grouped by pair; runs the two segment forms
    reaches: str = ""

    @property
    def name(self):
        return f"tri {self.label} z{self.z[0]}<-{self.z[1]} x{self.x[0]}<-{self.x[1]} y{self.y[0]}<-{self.y[1]} C{self.C}" + (" seg" if self.seg else "")

    @property
    def id(self):
        return self.name.replace(" ", "_")

    @property
    def fine(self):
        return self.z[0], self.x[0], self.y[0]

    @property
    def coarse(self):
        return self.z[1], self.x[1], self.y[1]

    @property
    def insts(self):
        """the kernel instantiations the GPU test launches for this case (the host test holds their union to INSTANTIATIONS)"""
        s = set()
        if self.C % 8 == 0:
            s |= {"fwd bf16->fp32", "fwd bf16->bf16", "bwd_rows bf16"}
        s |= {"fwd fp32->fp32", "bwd_rows fp32", "bwd atomic fp32"}
        if self.seg:
            s |= {"segmean bf16", "segmean fp32"}
        if self.C % 64 == 0 and self.C <= 256:
            s |= {f"{'gather_seg' if self.seg else 'gather'} {dt_name(dt)} CPL{self.C // 64}" for dt in (0, 1)}
        return s


# E1: three axes of step 1/4, so its forward outputs are odd multiples of 1/64 up to 8 in size and a bf16 store rounds them (a convex
# combination of |v| <= 8 on a coarser quantum never needs a ninth bit); the backward sums of every case grow past 8 and round.
_E = dict(E1=((17, 5), (9, 3), (13, 4)), E2=((5, 9), (9, 5), (13, 7)), E3=((7, 13), (5, 5), (2, 2)), E4=((1, 3), (4, 1), (9, 5)))
_G = dict(G1=((10, 5), (12, 6), (14, 7)), G2=((11, 4), (6, 11), (33, 17)))
TRI_EXACT = (
    [TriCase(k, *_E[k], C, True, reaches=why) for k, C, why in (("E1", 64, "CPL 1"), ("E2", 128, "CPL 2"), ("E3", 192, "CPL 3, upsampling axis"),
                                                                ("E4", 256, "CPL 4, extent-1 axes"), ("E1", 8, "one bf16 granule"), ("E2", 24, "CG = 3"))]
    + [TriCase(k, *_E[k], C, True, B=4, seg=True) for k, C in (("E1", 256), ("E2", 192), ("E3", 128), ("E4", 64), ("E2", 24))]
)
TRI_GENERAL = (
    [TriCase(k, *_G[k], C, False) for k, C in (("G1", 256), ("G2", 128), ("G1", 24), ("G2", 64), ("G1", 192))]
    + [TriCase(k, *_G[k], C, False, B=4, seg=True) for k, C in (("G1", 64), ("G2", 256), ("G1", 128), ("G2", 192), ("G2", 24))]
)
TRI = TRI_EXACT + TRI_GENERAL


@dataclasses.dataclass
class TriGeom:
    """points, the restated weights and the S1 row list of one case.  corner k = 4 (z upper) + 2 (x upper) + 1 (y upper)"""
    idx: np.ndarray             # int64 [N] flat fine index (x Yr + y) Zr + z
    pt_batch: np.ndarray        # int32 [N]
    w: np.ndarray               # float32 [N, 8] corner weights (wz * wx) * wy: the kernel's bits
    row: np.ndarray             # int64 [N, 8] flat coarse row ((b d + zi) h + xi) w + yi
    merged: np.ndarray          # bool [N]: an axis with i0 == i1 and t != 0
    rows1: np.ndarray           # int32 ascending: the corners of the occupied fine voxels (plain construction of S1)
    map1: np.ndarray            # int32 [B d h w]: rank in rows1 or -1
    nrows: int


def tri_points(c, idx, pt_batch):
    Zr, Xr, Yr = c.fine
    d, h, w = c.coarse
    zi, yi, xi = idx % Zr, (idx // Zr) % Yr, idx // (Zr * Yr)
    ax = [tri_axis(*p) for p in (c.z, c.x, c.y)]
    coord = (zi, xi, yi)
    W = np.empty((len(idx), 8), f32)
    R = np.empty((len(idx), 8), np.int64)
    one = f32(1)
    for k in range(8):
        up = (k & 4, k & 2, k & 1)
        wa, ia = [], []
        for a in range(3):
            i0, i1, t, _ = ax[a]
            wa.append((t[coord[a]] if up[a] else (one - t[coord[a]]).astype(f32)).astype(f32))
            ia.append((i1 if up[a] else i0)[coord[a]].astype(np.int64))
        W[:, k] = ((wa[0] * wa[1]).astype(f32) * wa[2]).astype(f32)
        R[:, k] = ((pt_batch.astype(np.int64) * d + ia[0]) * h + ia[1]) * w + ia[2]
    merged = np.zeros(len(idx), bool)
    for a in range(3):
        i0, i1, t, _ = ax[a]
        merged |= ((i0 == i1) & (t != 0))[coord[a]]
    nrows = c.B * d * h * w
    rows1 = np.unique(R.reshape(-1)).astype(np.int32)
    map1 = np.full(nrows, -1, np.int32)
    map1[rows1] = np.arange(len(rows1), dtype=np.int32)
    return TriGeom(idx.astype(np.int64), pt_batch.astype(np.int32), W, R, merged, rows1, map1, nrows)


def _occupied(c, r):
    """a random 40 % of each non-empty grid's fine voxels, the last voxel of every axis always among them; grid 1 stays empty.
    Points of grids 0, 1 (pair 0) come before those of grids 2, 3 (pair 1); inside a pair their order is random."""
    Zr, Xr, Yr = c.fine
    Vf = Zr * Xr * Yr
    idx, bat = [], []
    for b in range(c.B):
        if b == 1:
            continue
        pick = set(r.choice(Vf, size=max(1, int(round(0.4 * Vf))), replace=False).tolist()) | {Vf - 1, 0}
        pick = np.array(sorted(pick), np.int64)
        idx.append(pick)
        bat.append(np.full(len(pick), b, np.int32))
    idx, bat = np.concatenate(idx), np.concatenate(bat)
    pair = bat // 2 if c.seg else np.zeros_like(bat)
    order = np.concatenate([r.permutation(np.nonzero(pair == p)[0]) for p in range(int(pair.max()) + 1)])
    return idx[order], bat[order]


@dataclasses.dataclass
class SegPlan:
    """the first voxel-average round of one pair, as the kernels read it"""
    point_start: int
    n: int                      # points of the pair
    order: np.ndarray           # uint32 [n] local point indices, segment after segment
    starts: np.ndarray          # uint32 [nseg + 1]
    inv_seg: np.ndarray         # uint32 [n] local point -> segment
    inv_cnt: np.ndarray         # float32 [n] 1 / size of the point's segment
    row_off: int                # first row of the pair in g1 / the concatenated outputs

    @property
    def nseg(self):
        return len(self.starts) - 1


def _plans(c, bat, r):
    plans, row_off = [], 0
    sizes_from = (1, 2, 4, 8) if c.exact else (1, 2, 3, 4, 5, 6, 7, 8)
    for p in range(c.B // 2):
        loc = np.nonzero(bat // 2 == p)[0]
        n, sizes = len(loc), []
        while sum(sizes) < n:
            s = int(r.choice(sizes_from))
            sizes.append(s if sum(sizes) + s <= n else 1)
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        order = r.permutation(n).astype(np.uint32)
        inv_seg = np.empty(n, np.uint32)
        inv_cnt = np.empty(n, f32)
        for sgm, (a, b) in enumerate(zip(starts[:-1], starts[1:])):
            inv_seg[order[a:b]] = sgm
            inv_cnt[order[a:b]] = f32(1) / f32(b - a)
        plans.append(SegPlan(int(loc[0]), n, order, starts, inv_seg, inv_cnt, row_off))
        assert np.array_equal(loc, np.arange(loc[0], loc[0] + n))
        row_off += len(sizes)
    return plans


@functools.lru_cache(maxsize=4)
def tri_operands(c):
    """geom, p1 [B, d, h, w, C] fp64 per dtype (values the dtype holds), dfeat [N, C] fp64 (fp32 values), and for seg cases the plans and g1"""
    r = _rng(c.name)
    idx, bat = _occupied(c, r)
    geom = tri_points(c, idx, bat)
    shape = (c.B, *c.coarse, c.C)
    Npt = len(idx)
    if c.exact:
        p1 = _t(r.randint(-8, 9, size=shape))
        o = dict(p1={0: p1, 1: p1}, dfeat=_t(r.randint(-8, 9, size=(Npt, c.C))))
    else:
        p = _t(r.randn(*shape).astype(f32))
        o = dict(p1={0: rounded(p, 0), 1: p}, dfeat=_t(r.randn(Npt, c.C).astype(f32)))
    o["geom"] = geom
    if c.seg:
        o["plans"] = _plans(c, bat, r)
        rows = sum(p.nseg for p in o["plans"])
        o["g1"] = _t(r.randint(-8, 9, size=(rows, c.C))) if c.exact else _t(r.randn(rows, c.C).astype(f32))
    return o


def tri_forward(geom, p1):
    """(out64 [N, C], sum_c |w_c v_c| [N, C]) from the restated weights; p1 [B, d, h, w, C] fp64"""
    flat = p1.reshape(-1, p1.shape[-1])
    out = torch.zeros(len(geom.idx), flat.shape[1], dtype=F64)
    mag = torch.zeros_like(out)
    for k in range(8):
        t = flat[torch.from_numpy(geom.row[:, k])] * _t(geom.w[:, k])[:, None]
        out += t
        mag += t.abs()
    return out, mag


def tri_segment_mean(plan, out64, mag):
    """per segment of one pair: (mean64, sum over members of mag, member count) — rows in segment order"""
    members = torch.from_numpy(plan.order.astype(np.int64)) + plan.point_start
    seg_of = torch.from_numpy(np.repeat(np.arange(plan.nseg), np.diff(plan.starts.astype(np.int64))))
    cnt = torch.from_numpy(np.diff(plan.starts.astype(np.int64))).double()
    s = torch.zeros(plan.nseg, out64.shape[1], dtype=F64).index_add_(0, seg_of, out64[members])
    m = torch.zeros_like(s).index_add_(0, seg_of, mag[members])
    return s / cnt[:, None], m, cnt


def seg_dfeat(plans, g1, Npt):
    """d feats[n] = g1[inv_seg[n] + row_off] * inv_cnt[n] in fp64 (inv_cnt is the fp32 value the kernel reads)"""
    out = torch.zeros(Npt, g1.shape[1], dtype=F64)
    for p in plans:
        rows = torch.from_numpy(p.inv_seg.astype(np.int64) + p.row_off)
        out[p.point_start:p.point_start + p.n] = g1[rows] * _t(p.inv_cnt)[:, None]
    return out


def tri_backward(geom, dfeat):
    """the fp64 scatter: (dp64 [rows, C], sum |w g| [rows, C], K [rows] corner terms with w != 0, sum |w g| over the terms of merged points)"""
    C = dfeat.shape[1]
    dp = torch.zeros(geom.nrows, C, dtype=F64)
    mag, mag_m = torch.zeros_like(dp), torch.zeros_like(dp)
    K = torch.zeros(geom.nrows, dtype=F64)
    merged = torch.from_numpy(geom.merged).double()[:, None]
    for k in range(8):
        rows = torch.from_numpy(geom.row[:, k])
        t = dfeat * _t(geom.w[:, k])[:, None]
        dp.index_add_(0, rows, t)
        mag.index_add_(0, rows, t.abs())
        mag_m.index_add_(0, rows, t.abs() * merged)
        K.index_add_(0, rows, _t(geom.w[:, k] != 0))
    return dp, mag, K, mag_m


def tri_backward_bound(dp, mag, K, mag_m, dt, seg=False, gather=False):
    """see the module docstring: g_(K + 1) sum|w g| (+ one rounding per term for SEG, + g_(7) on merged terms for the gather forms) + BFU |dp64|"""
    n = K + 1 + (1 if seg else 0)
    e = (n * U / (1 - n * U))[:, None] * mag
    if gather:
        e = e + g_(7) * mag_m
    return e + (BFU * dp.abs() if dt == 0 else 0.0)


def sweep_case(axis, n_out, n_in):
    """one axis varies, the other two have extent 1; every fine voxel occupied, every coarse voxel a row; C = 64"""
    pairs = [(1, 1)] * 3
    pairs[axis] = (n_out, n_in)
    return TriCase(f"sweep{axis}", *pairs, 64, False, B=1)


def sweep_operands(c):
    Vf = c.fine[0] * c.fine[1] * c.fine[2]
    geom = tri_points(c, np.arange(Vf, dtype=np.int64), np.zeros(Vf, np.int32))
    geom.rows1 = np.arange(geom.nrows, dtype=np.int32)
    geom.map1 = np.arange(geom.nrows, dtype=np.int32)
    return geom, _t(_rng(c.name).randn(Vf, 64).astype(f32))


# ================================================================================================ 5. entry checks
class _Dummy:
    buf = (ctypes.c_longlong * 8)()
    addr = ctypes.addressof(buf)


# (what, entry, C, dtype, extra): every call must return DREG_EINVAL (-1) with null buffers, before any launch
EINVAL = [
    ("C % 8 bf16", "maxpool_fwd", 12, 0, None), ("C % 4 fp32", "maxpool_fwd", 6, 1, None),
    ("C % 8 bf16", "maxpool_bwd_acc", 12, 0, None), ("C % 4 fp32", "maxpool_bwd_acc", 6, 1, None),
    ("C % 8 bf16", "maxpool_bwd", 12, 0, None), ("C % 4 fp32", "maxpool_bwd", 6, 1, None),
    ("C % 8 bf16", "downsample_sum", 12, 0, None), ("C % 4 fp32", "downsample_sum", 6, 1, None),
    ("C % 8 bf16", "downsample_sum_rows", 12, 0, None),
    ("C % 8 bf16", "gather_fwd", 12, 0, None), ("C % 4 fp32", "gather_fwd", 6, 1, None), ("C % 8 bf16 out", "gather_fwd_bf16out", 12, 0, None),
    ("C % 8 bf16", "bwd_rows", 12, 0, None),
    ("C % 64", "bwd_gather", 96, 0, None), ("C > 256", "bwd_gather", 320, 1, None),
    ("C % 64", "bwd_gather_rows_only", 96, 1, None), ("C > 256", "bwd_gather_rows_only", 320, 0, None),
    ("C % 64", "bwd_gather_seg", 96, 0, "descs"), ("C > 256", "bwd_gather_seg", 320, 1, "descs"),
    ("null seg_descs", "bwd_gather_seg", 64, 0, None),
    ("C % 4", "segment_mean", 6, 1, None), ("negative point_start", "segment_mean", 64, 0, "negative"),
    ("C % 8", "stem_fwd", 12, 0, None), ("C % 8", "stem_bwd", 12, 0, None),
    ("ragged last slab C 2056, training", "stem_fwd", 2056, 0, None),
]


def refused_call(lib, entry, C, dt, extra, stream=None):
    """one call of the EINVAL table: 2 grids of a 4^3 volume pooled / downsampled to 2^3, 5 points, 3 rows; every buffer null"""
    z = None
    geo = (2, 4, 4, 4, 2, 2, 2)
    if entry == "maxpool_fwd":
        return lib.dreg_maxpool3d_fwd(z, z, z, *geo, C, dt, stream)
    if entry == "maxpool_bwd_acc":
        return lib.dreg_maxpool3d_bwd_acc(z, z, z, *geo, C, 1, dt, stream)
    if entry == "maxpool_bwd":
        return lib.dreg_maxpool3d_bwd(z, z, z, *geo, C, dt, stream)
    if entry == "downsample_sum":
        return lib.dreg_downsample_sum(z, z, *geo, C, dt, stream)
    if entry == "downsample_sum_rows":
        return lib.dreg_downsample_sum_rows(z, z, z, 3, *geo[1:], C, dt, stream)
    if entry in ("gather_fwd", "gather_fwd_bf16out"):
        return lib.dreg_trilinear_gather_fwd(z, z, z, z, 5, 2, 2, 2, C, 4, 4, 4, dt, int(entry == "gather_fwd"), stream)
    if entry == "bwd_rows":
        return lib.dreg_trilinear_gather_bwd_rows(z, z, z, z, 3, z, z, z, 5, 2, 2, 2, 2, C, 4, 4, 4, dt, stream)
    tail = (5, 2, 2, 2, 2, C, 4, 4, 4, dt)
    if entry == "bwd_gather":
        return lib.dreg_trilinear_gather_bwd_gather(z, z, z, z, 3, z, z, *tail, stream)
    if entry == "bwd_gather_rows_only":
        return lib.dreg_trilinear_gather_bwd_gather_rows_only(z, z, z, z, 3, z, z, *tail, stream)
    if entry == "bwd_gather_seg":
        return lib.dreg_trilinear_gather_bwd_gather_seg(z, _Dummy.addr if extra == "descs" else None, z, z, z, 3, z, z, *tail, 1, stream)
    if entry == "segment_mean":
        return lib.dreg_gather_segment_mean(z, z, z, -1 if extra == "negative" else 0, z, z, z, z, 3, 2, 2, 2, C, 4, 4, 4, dt, stream)
    if entry == "stem_fwd":
        return lib.dreg_bn_relu_maxpool_fwd(z, z, z, z, z, z, z, z, z, z, *geo, C, N.EPS, N.MOM, 1, 1, stream)
    if entry == "stem_bwd":
        return lib.dreg_bn_relu_maxpool_bwd(z, z, z, z, z, z, z, z, z, z, *geo, C, 1, 0, stream)
    raise AssertionError(entry)
