"""Integer-operand cases for the convolution kernels of csrc/conv.hip, and their fp64 references (no GPU).

With small integers in bf16 every product and every fp32 partial sum of a convolution is an exact integer below 2^24, so the result does
not depend on the accumulation order, the tile shape, the split count or the MFMA shape: it equals the fp64 reference exactly (fp32 outputs)
or its round-to-nearest-even bf16 (bf16 outputs; f2bf in csrc/common.h).  tests/test_conv_exact_host.py checks the table (each case reaches
the instantiation it names; the preconditions of exactness hold on the reference alone), tests/test_hip_conv_exact.py runs it.

A case is written in the LAYER's terms (input volume `din`, cin -> cout, k, stride, pad) whichever pass it runs; `variant` is the code
dreg_conv3d_igemm_variant / dreg_conv3d_wgrad_variant / *_group_fill must return for the launch (None where those cannot express it: the
fp32 / use_tr = 0 weight gradients, an empty row list).  Operands are int8 on the host, drawn per (geometry, amp, seed) and cached at module
scope with the references, so the knob variants of a shape share one of each.  `amp` (operands in [-amp, amp], 30 % zeros) is chosen per K so
that bf16 outputs exceed 256 often enough to be rounded (asserted in the host test)."""
import dataclasses
import functools
import zlib

import torch
import torch.nn.functional as F

SENTINEL = 77.0            # what the rows a launch must not touch hold beforehand (exact in bf16)
ZERO_SHARE = 0.3
LIMIT = 1 << 24


def odim(i, k, s, p):
    return (i + 2 * p - k) // s + 1


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    api: str                  # fwd | fwd_occ | rows | bnstats | defer | dgrad | dgrad_s2 | wgrad | wgrad_occ | wgrad_rows | wgrad_partials | group | halo | halo_dgrad | brick
    B: int
    din: tuple
    cin: int                  # input channels as stored (padded)
    cout: int
    k: int
    s: int = 1
    pad: int = -1             # -1: k // 2
    cin_real: int = 0         # 0: cin
    dt: int = 0               # 0 bf16, 1 fp32
    out_f32: bool = False
    bias: bool = False
    relu: bool = False
    addend: str = ""          # "", "same", "up2"
    ws: bool = True           # forward: pass the split-K workspace
    nrows: int = -1           # row-list length (-1: dense)
    acc: bool = False         # accumulate into an existing dw / dIn
    use_tr: int = 1
    amp: int = 3
    seed: int = 0
    knobs: tuple = ()         # ((setter, value, default), ...) on the measurement build
    variant: object = None
    ragged: int = 0           # the row count must NOT be a multiple of this tile height (0: nothing claimed)
    linear: bool = False      # group: through dreg_linear_wgrad_group_fill

    @property
    def p(self):
        return self.k // 2 if self.pad < 0 else self.pad

    @property
    def creal(self):
        return self.cin_real or self.cin

    @property
    def dout(self):
        return tuple(odim(d, self.k, self.s, self.p) for d in self.din)

    @property
    def M(self):
        do = self.dout
        return self.B * do[0] * do[1] * do[2]

    @property
    def key(self):
        """what the operands and the references depend on"""
        return (self.B, self.din, self.cin, self.creal, self.cout, self.k, self.s, self.p, self.amp, self.seed, self.api in ("fwd_occ", "wgrad_occ"))

    @property
    def id(self):
        return self.name.replace(" ", "_")


# ------------------------------------------------------------------------------------------------ operands
def _gen(key, what):
    return torch.Generator().manual_seed(zlib.crc32(repr((key, what)).encode()))


def ints(gen, shape, amp):
    """int8 in [-amp, amp], ZERO_SHARE of them forced to zero"""
    v = torch.randint(-amp, amp + 1, shape, generator=gen, dtype=torch.int8)
    v[torch.rand(shape, generator=gen) < ZERO_SHARE] = 0
    return v


class Operands:
    """small-integer host tensors (int8; the bias int16) of one geometry, made on first use, each from its own seed (so none depends on which others a test asked for):
    x [B,D,H,W,cin] (padding channels zero, as the callers leave them: regtr.pack_grids, F.pad), w [cout,cin_real,k,k,k], bias [cout],
    g [B,Do,Ho,Wo,cout], add_same [B,Do,Ho,Wo,cout], add_up [B,ceil(Do/2),..,cout], dw0 [cout,cin_real,k^3], din0 [B,D,H,W,cin],
    inocc uint8 [B,D,H] (occupancy cases: x is zero on the W-rows flagged 0)."""

    def __init__(self, key):
        self.key = key
        self.B, self.din, self.cin, self.creal, self.cout, self.k, self.s, self.p, self.amp, _, self.occ = key
        self.dout = tuple(odim(d, self.k, self.s, self.p) for d in self.din)
        self._t = {}

    def _make(self, what):
        g, a = _gen(self.key, what), self.amp
        B, cin, cout = self.B, self.cin, self.cout
        if what == "inocc":
            # 90 % of the W-rows of the first 0.6 D planes, none behind them: the last output planes see no occupied row at all
            v = (torch.rand(B, *self.din[:2], generator=g) < 0.9).to(torch.uint8)
            v[:, -(-6 * self.din[0] // 10):] = 0
            v[:, 0, 0] = 1
            return v
        if what == "x":
            v = ints(g, (B, *self.din, cin), a)
            v[..., self.creal:] = 0
            if self.occ:
                v = v * self.get("inocc")[..., None, None].to(torch.int8)
            return v
        if what == "w":
            return ints(g, (cout, self.creal, self.k, self.k, self.k), a)
        if what == "bias":           # 0 .. 32 amp: lifts the pre-activations by a fraction of their spread, so that a ReLU keeps more than half of them
            return torch.randint(0, 32 * a + 1, (cout,), generator=g, dtype=torch.int16)
        if what == "g":
            return ints(g, (B, *self.dout, cout), a)
        if what == "add_same":
            return ints(g, (B, *self.dout, cout), a)
        if what == "add_up":
            return ints(g, (B, *((d + 1) // 2 for d in self.dout), cout), a)
        if what == "dw0":
            return ints(g, (cout, self.creal, self.k ** 3), a)
        if what == "din0":
            return ints(g, (B, *self.din, cin), a)
        raise KeyError(what)

    def get(self, what):
        if what not in self._t:
            self._t[what] = self._make(what)
        return self._t[what]


@functools.lru_cache(maxsize=None)
def _operands(key):
    return Operands(key)


def operands(case):
    return _operands(case.key)


@functools.lru_cache(maxsize=None)
def _rows(key, nrows):
    o = _operands(key)
    M = o.B * o.dout[0] * o.dout[1] * o.dout[2]
    if nrows == 0:
        return torch.zeros(0, dtype=torch.int32)
    r = torch.randperm(M, generator=_gen(key, ("rows", nrows)))[:nrows]
    r[0], r[1] = 0, M - 1                      # the first and the last voxel of the launch are always in the list
    r = torch.unique(r)
    return r.sort().values.int()


def rows(case):
    """ascending int32 row list of a row-list case (its length may fall one short of case.nrows when the forced ends collide)"""
    return _rows(case.key, case.nrows)


# ------------------------------------------------------------------------------------------------ fp64 references
def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _store(exact):
    """references are integers below 2^24: kept as fp32 (lossless, asserted) to halve the cache"""
    f = exact.float()
    assert torch.equal(f.double(), exact)
    return f


@functools.lru_cache(maxsize=None)
def _conv(key):
    o = _operands(key)
    x = _ncdhw(o.get("x")[..., :o.creal].double())
    return _store(_ndhwc(F.conv3d(x, o.get("w").double(), stride=o.s, padding=o.p)))


def up2(a, dout):
    for d in (1, 2, 3):
        a = a.repeat_interleave(2, dim=d)
    return a[:, :dout[0], :dout[1], :dout[2]]


def fwd_exact(case):
    """[B,Do,Ho,Wo,cout] fp64: conv + bias + addend (same-size, or nearest x2 upsampled and cropped), then ReLU"""
    o = operands(case)
    y = _conv(case.key).double()
    if case.bias:
        y = y + o.get("bias").double()
    if case.addend == "same":
        y = y + o.get("add_same").double()
    elif case.addend == "up2":
        y = y + up2(o.get("add_up").double(), case.dout)
    return y.clamp_min(0) if case.relu else y


@functools.lru_cache(maxsize=None)
def _dgrad(key):
    o = _operands(key)
    g = _ncdhw(o.get("g").double())
    dx = torch.nn.grad.conv3d_input((o.B, o.creal, *o.din), o.get("w").double(), g, stride=o.s, padding=o.p)
    return _store(_ndhwc(dx))


def dgrad_exact(case):
    """[B,D,H,W,cin_real] fp64: the data gradient of the layer for upstream gradient g (+ din0 when the case accumulates)"""
    d = _dgrad(case.key).double()
    return d + operands(case).get("din0")[..., :case.creal].double() if case.acc else d


@functools.lru_cache(maxsize=None)
def _wgrad(key, nrows):
    """tap by tap: dw[:, :, t] = g^T x_shifted over the rows of the launch (all, or the row list)"""
    o = _operands(key)
    k, s, p = o.k, o.s, o.p
    Do, Ho, Wo = o.dout
    M = o.B * Do * Ho * Wo
    sel = None if nrows < 0 else _rows(key, nrows).long()
    g = o.get("g").reshape(M, o.cout)
    g = (g if sel is None else g[sel]).double().t().contiguous()
    xp = F.pad(o.get("x")[..., :o.creal], (0, 0, p, p, p, p, p, p))
    dw = torch.zeros(o.cout, o.creal, k ** 3, dtype=torch.float64)
    for t in range(k ** 3):
        kd, kh, kw = t // (k * k), (t // k) % k, t % k
        xs = xp[:, kd:kd + s * (Do - 1) + 1:s, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s].reshape(M, o.creal)
        xs = (xs if sel is None else xs[sel]).double()
        dw[:, :, t] = g @ xs
    return _store(dw)


def wgrad_exact(case):
    """[cout, cin_real, k^3] fp64 (+ dw0 when the case accumulates); row-list cases sum over the listed rows only"""
    d = _wgrad(case.key, case.nrows).double()
    return d + operands(case).get("dw0").double() if case.acc else d


def bn_sums_exact(case):
    """[B, V / 128, cout, 2] fp64: per 128-row chunk the sum and the sum of squares of the STORED bf16 output"""
    y = fwd_exact(case).float().bfloat16().double()
    V = case.M // case.B
    y = y.reshape(case.B, V // 128, 128, case.cout)
    return torch.stack((y.sum(2), (y * y).sum(2)), dim=-1)


def worst_sum(case):
    """an upper bound of sum |a||b| + |epilogue terms| over every output of the case, from the operand range alone"""
    a2 = case.amp * case.amp
    if case.api in ("wgrad", "wgrad_occ", "wgrad_rows", "wgrad_partials", "group"):
        return (case.M if case.nrows < 0 else case.nrows) * a2 + (case.amp if case.acc else 0)
    if case.api in ("dgrad", "dgrad_s2", "halo_dgrad"):
        return case.k ** 3 * case.cout * a2 + (case.amp if case.acc else 0)
    return case.k ** 3 * case.creal * a2 + (32 * case.amp if case.bias else 0) + (case.amp if case.addend else 0)


# ------------------------------------------------------------------------------------------------ which instantiation a case runs
def variant_query(lib, c):
    """the host-only label of the launch case c makes (None where the label functions cannot express it)"""
    if c.api in ("fwd", "fwd_occ", "rows", "bnstats", "defer"):
        if c.api == "rows" and c.nrows == 0:
            return None
        return lib.dreg_conv3d_igemm_variant(c.B, *c.din, c.cin, *c.dout, c.cout, c.k, c.s, c.p, 0, max(c.nrows, 0), int(c.ws and c.api != "rows"),
                                             int(bool(c.addend)), c.dt)
    if c.api == "dgrad":       # the gathered operand is g: the launch's Cin is the layer's cout
        return lib.dreg_conv3d_igemm_variant(c.B, *c.dout, c.cout, *c.din, c.creal, c.k, c.s, c.p, 1, 0, int(c.ws), 0, c.dt)
    if c.api == "dgrad_s2":    # one 2^3-tap (or 1-tap) convolution over g onto the class lattice, 8 x cin (or cin) output channels
        lat = tuple((d + 1) // 2 for d in c.din)
        ncls = 1 if c.k == 1 else 8
        return lib.dreg_conv3d_igemm_variant(c.B, *c.dout, c.cout, *lat, ncls * c.cin, 1 if c.k == 1 else 2, 1, 0, 0, 0, 0, int(c.acc), 0)
    if c.api == "group":
        import ctypes
        desc = (ctypes.c_uint8 * lib.dreg_wgrad_group_desc_bytes())()
        var, nblk = ctypes.c_int(0), ctypes.c_int(0)
        nws = lib.dreg_conv3d_wgrad_workspace_bytes(c.B, *c.dout, c.cin, c.cout, c.k, 0)
        if c.linear:
            rc = lib.dreg_linear_wgrad_group_fill(desc, None, None, None, nws, c.B, c.cin, c.cout, ctypes.byref(var), ctypes.byref(nblk))
        else:
            rc = lib.dreg_conv3d_wgrad_group_fill(desc, None, None, None, nws, c.B, *c.din, c.cin, *c.dout, c.cout, c.k, c.s, c.p, ctypes.byref(var), ctypes.byref(nblk))
        return var.value if rc == 0 else -1
    if c.dt != 0 or not c.use_tr:
        return None
    return lib.dreg_conv3d_wgrad_variant(c.B, *c.dout, c.cin, c.cout, c.k, int(c.nrows >= 0), max(c.nrows, 0), int(c.api == "wgrad_occ"))


def row_occupancy_exact(case):
    """uint8 [B,Do,Ho]: 1 where the window of output row (zo, ho, *) holds an occupied input row (dreg_conv_row_occupancy)"""
    occ = operands(case).get("inocc").float()[:, None]
    return F.max_pool2d(occ, case.k, case.s, case.p)[:, 0].to(torch.uint8)


def wgrad_kind(c):
    return "group" if c.api == "group" else ("rows" if c.nrows >= 0 else ("occ" if c.api == "wgrad_occ" else "dense"))


# ------------------------------------------------------------------------------------------------ the table
# volumes: pairwise different, non-power-of-two output dims (magic division), B > 1 where the row threshold allows it
SMALL = (7, 9, 10)          # 630 voxels per grid: split-K (fewer than 128 tiles at the nominal batch of 8)
MID = (11, 13, 14)          # 2,002 voxels: 32 row tiles at B = 2, the anti-phase 128-row forms
WIDE = (23, 27, 29)         # 18,009 rows: 141 row tiles, past the anti-phase limit of 256 tiles at 256 output channels
LONG = (31, 33, 35)         # 35,805 rows: 280 row tiles, past it at 64 output channels too
HUGE = (65, 33, 31)         # 66,495 rows >= 65,536: the 256-row tiles, ragged (66,495 = 259 x 256 + 191)
POW = (64, 32, 32)          # 65,536 rows with Wo % 32 == 0: the lean ("fast") loop of the dense 8-wave weight gradient
STEM = (17, 13, 16)         # k 5 / stride 2 / pad 2 -> 9 x 7 x 8 (Wo divides 128: whole W-rows per tile, which the occupancy form needs)
ODD = (13, 11, 9)           # stride 2 -> 7 x 6 x 5: a ragged parity-class lattice on every axis

G0, G3 = ("dreg_conv_set_glds", 0, 1), ("dreg_conv_set_glds", 3, 1)
AP0, AP256_0 = ("dreg_conv_set_igemm_ap", 0, 256), ("dreg_conv_set_igemm_ap256", 0, 1)
NARROW0 = ("dreg_conv_set_narrow_small", 0, 2)


def stages(n):
    return ("dreg_conv_set_glds_stages", n, 0)


def big(n):
    return ("dreg_conv_set_wgrad_big", n, 3)


def ring(n):
    return ("dreg_conv_set_wgrad_ring", n, 3)


PIPE1 = ("dreg_conv_set_wgrad_pipe", 1, 0)
ROWS_FAST0 = ("dreg_conv_set_wgrad_rows_fast", 0, 1)
ROW_SPLITS0 = ("dreg_conv_set_row_splits", 0, 1)

# igemm code: kind * 1e8 + BM * 1e5 + BN * 100 + AP * 10 + splitK
FWD = [
    # split-K, finished by splitk_reduce_kernel with bias + ReLU: both widths, anti-phase (<= 256 workgroups) and four-wave
    Case("splitk ap 128x128 bias relu", "fwd", 2, SMALL, 256, 256, 3, bias=True, relu=True, variant=12812811, ragged=128),
    Case("splitk ap 128x64 bias relu", "fwd", 2, SMALL, 256, 64, 3, bias=True, relu=True, variant=12806411, ragged=128),
    Case("splitk four-wave 128x128 bias relu", "fwd", 9, SMALL, 256, 256, 3, bias=True, relu=True, variant=12812801, ragged=128),
    Case("splitk four-wave 128x64 fp32 out", "fwd", 9, SMALL, 256, 64, 3, bias=True, out_f32=True, variant=12806401, ragged=128),
    Case("splitk deferred", "defer", 2, SMALL, 256, 256, 3, variant=12812811, ragged=128),
    Case("splitk refused by an addend", "fwd", 2, SMALL, 256, 256, 3, addend="same", bias=True, variant=12812810, ragged=128),
    Case("no workspace no splitk", "fwd", 2, SMALL, 256, 256, 3, ws=False, bias=True, relu=True, variant=12812810, ragged=128),
    Case("bnstats on a splitk launch", "bnstats", 2, SMALL, 256, 256, 3, variant=12812811),
    # the 256 x 256 tile and its neighbours on >= 65,536 rows
    Case("256x256 ap ragged", "fwd", 1, HUGE, 64, 256, 3, bias=True, amp=4, variant=25625610, ragged=256),
    Case("256x256 lockstep", "fwd", 1, HUGE, 64, 256, 3, bias=True, amp=4, knobs=(AP256_0,), variant=25625600, ragged=256),
    Case("128x256", "fwd", 1, HUGE, 64, 256, 3, bias=True, amp=4, knobs=(G3,), variant=12825600, ragged=128),
    Case("pointwise read-modify-write", "fwd", 1, HUGE, 64, 256, 1, addend="same", amp=9, variant=12812800, ragged=128),
    # 128-row tiles
    Case("ap 128x128 up2 addend bias relu", "fwd", 2, MID, 128, 128, 3, addend="up2", bias=True, relu=True, variant=12812810, ragged=128),
    Case("ap 128x64 fp32 out same addend", "fwd", 2, MID, 128, 64, 3, addend="same", out_f32=True, variant=12806410, ragged=128),
    Case("four-wave 128x128", "fwd", 1, WIDE, 64, 256, 3, amp=4, bias=True, relu=True, variant=12812800, ragged=128),
    Case("four-wave 128x128 3 stages", "fwd", 1, WIDE, 64, 256, 3, amp=4, bias=True, relu=True, knobs=(stages(3),), variant=12812800, ragged=128),
    Case("four-wave 128x128 4 stages", "fwd", 1, WIDE, 64, 256, 3, amp=4, bias=True, relu=True, knobs=(stages(4),), variant=12812800, ragged=128),
    Case("four-wave 128x64", "fwd", 1, LONG, 64, 64, 3, amp=4, bias=True, variant=12806400, ragged=128),
    Case("igemm_ap 0 narrow 128x64", "fwd", 2, MID, 128, 128, 3, addend="up2", bias=True, relu=True, knobs=(AP0,), variant=12806400, ragged=128),
    Case("igemm_ap 0 narrow_small 0", "fwd", 2, MID, 128, 128, 3, addend="up2", bias=True, relu=True, knobs=(AP0, NARROW0), variant=12812800, ragged=128),
    Case("glds 0 register-staged 128", "fwd", 2, MID, 128, 128, 3, addend="up2", bias=True, relu=True, knobs=(G0,), variant=112812800, ragged=128),
    # the register-staged kernel at defaults: the stem (4 real channels of 8, Kpad 1000 -> 1024) and the fp32 path
    Case("stem k5 s2", "fwd", 2, STEM, 8, 64, 5, 2, 2, cin_real=4, amp=5, bias=True, relu=True, variant=112806400, ragged=128),
    Case("stem k5 s2 occupancy", "fwd_occ", 2, STEM, 8, 64, 5, 2, 2, cin_real=4, amp=6, variant=112806400, ragged=128),
    Case("fp32 register-staged 128", "fwd", 2, SMALL, 64, 128, 3, dt=1, bias=True, relu=True, variant=112812800, ragged=128),
    Case("fp32 register-staged 64 same addend", "fwd", 2, SMALL, 64, 64, 3, dt=1, addend="same", variant=112806400, ragged=128),
    # row lists
    Case("rows direct-to-LDS", "rows", 2, MID, 128, 128, 3, nrows=1500, bias=True, relu=True, variant=12812810, ragged=128),
    Case("rows direct-to-LDS fp32 out up2", "rows", 2, MID, 128, 128, 3, nrows=1500, addend="up2", out_f32=True, variant=12812810, ragged=128),
    Case("rows stem", "rows", 2, STEM, 8, 64, 5, 2, 2, cin_real=4, amp=5, nrows=300, bias=True, variant=112806400, ragged=128),
    Case("rows empty", "rows", 2, MID, 128, 128, 3, nrows=0),
    # BatchNorm sums from the epilogue (V = 2,304 = 18 chunks of 128 rows per grid: at 2,048 voxels and more a 128-channel layer no longer splits K)
    Case("bnstats 128x128", "bnstats", 2, (8, 12, 24), 128, 128, 3, variant=12812810),
]

DGRAD = [
    Case("dgrad s1 ap 128x128", "dgrad", 2, (12, 13, 14), 128, 128, 3, variant=12812810, ragged=128),
    Case("dgrad s1 splitk", "dgrad", 2, SMALL, 256, 256, 3, variant=12812811, ragged=128),
    Case("dgrad_s2 k3 odd dims", "dgrad_s2", 2, ODD, 64, 128, 3, 2, amp=5, variant=12812810, ragged=128),
    Case("dgrad_s2_acc k3 odd dims", "dgrad_s2", 2, ODD, 64, 128, 3, 2, amp=5, acc=True, variant=12812810, ragged=128),
    Case("dgrad_s2 k1 odd dims", "dgrad_s2", 2, ODD, 64, 128, 1, 2, 0, amp=7, variant=12806410, ragged=128),
    Case("dgrad_s2_acc k1 odd dims", "dgrad_s2", 2, ODD, 64, 128, 1, 2, 0, amp=7, acc=True, variant=12806410, ragged=128),
]

# weight-gradient code: BM * 1000 + BNC (+ 1,000,000: the register-staged kernel)
D8 = dict(B=1, din=POW, cin=256, cout=256, k=1)      # the dense 8-wave tile on 256 -> 256, 1^3
WGRAD = [
    Case("wgrad dense8 fast", "wgrad", variant=256256, **D8),
    Case("wgrad dense8 fast Kpad 1728", "wgrad", 1, POW, 64, 256, 3, variant=256256),
    Case("wgrad dense8 general loop ragged Kpad 1728", "wgrad", 1, HUGE, 64, 256, 3, variant=256256, ragged=256),
    Case("wgrad four-wave 128x128", "wgrad", 2, WIDE, 256, 256, 1, variant=128128, ragged=128),
    Case("wgrad four-wave 128x64 empty last splits", "wgrad", 2, (15, 21, 23), 256, 256, 1, variant=128064, ragged=128),
    Case("wgrad four-wave 64x128", "wgrad", 2, (15, 21, 23), 64, 64, 3, variant=64128, ragged=64),
    Case("wgrad four-wave 64x64 accumulate", "wgrad", 3, (3, 5, 7), 64, 64, 1, acc=True, variant=64064, ragged=64),
    Case("wgrad narrow rule linear", "wgrad", 9859, (1, 1, 1), 256, 256, 1, variant=64064, ragged=64),
    Case("wgrad stem", "wgrad", 2, STEM, 8, 64, 5, 2, 2, cin_real=4, variant=64064, ragged=64),
    Case("wgrad occupancy flags", "wgrad_occ", 2, (5, 7, 64), 64, 64, 3, variant=64064),
    Case("wgrad rows four-wave", "wgrad_rows", 2, MID, 128, 128, 3, nrows=1500, variant=64064, ragged=64),
    Case("wgrad rows four-wave accumulate", "wgrad_rows", 2, MID, 128, 128, 3, nrows=1500, acc=True, variant=64064, ragged=64),
    Case("wgrad rows 8-wave anti-phase", "wgrad_rows", 2, LONG, 256, 256, 3, nrows=20000, variant=256256, ragged=256),
    Case("wgrad fp32", "wgrad", 2, SMALL, 64, 64, 3, dt=1, use_tr=0, ragged=64),
    Case("wgrad bf16 use_tr 0", "wgrad", 2, SMALL, 64, 64, 3, use_tr=0, ragged=64),
    Case("wgrad partials batched reduce accumulate", "wgrad_partials", 2, (15, 21, 23), 64, 64, 3, acc=True, variant=64128, ragged=64),
    Case("wgrad partials rows fewer slices", "wgrad_partials", 2, MID, 128, 128, 3, nrows=1500, acc=True, variant=64064, ragged=64),
    # knob-only forms
    Case("wgrad glds 0 register-staged", "wgrad", 2, WIDE, 256, 256, 1, knobs=(G0,), variant=1128128, ragged=128),
    Case("wgrad_big 0 four-wave narrow", "wgrad", knobs=(big(0),), variant=128064, **D8),
    Case("wgrad_big 1 256x128", "wgrad", knobs=(big(1),), variant=256128, **D8),
    Case("wgrad_ring 0", "wgrad", knobs=(ring(0),), variant=256256, **D8),
    Case("wgrad_ring 1", "wgrad", knobs=(ring(1),), variant=256256, **D8),
    Case("wgrad_ring 2", "wgrad", knobs=(ring(2),), variant=256256, **D8),
    Case("wgrad_ring 8", "wgrad", knobs=(ring(8),), variant=256256, **D8),
    Case("wgrad_ring 0 wgrad_pipe 1", "wgrad", knobs=(ring(0), PIPE1), variant=256256, **D8),
    Case("wgrad_pipe 1 Kpad 1728 four-wave", "wgrad", 1, POW, 64, 256, 3, knobs=(PIPE1,), variant=128128),
    Case("wgrad_rows_fast 0 four-wave", "wgrad_rows", 2, MID, 128, 128, 3, nrows=1500, knobs=(ROWS_FAST0,), variant=64064, ragged=64),
    Case("wgrad_rows_fast 0 20000 rows", "wgrad_rows", 2, LONG, 256, 256, 3, nrows=20000, knobs=(ROWS_FAST0,), variant=128128, ragged=128),
    Case("row_splits 0 20000 rows", "wgrad_rows", 2, LONG, 256, 256, 3, nrows=20000, knobs=(ROW_SPLITS0,), variant=256256, ragged=256),
    Case("narrow_small 0 linear", "wgrad", 9859, (1, 1, 1), 256, 256, 1, knobs=(NARROW0,), variant=128128, ragged=128),
]

# grouped launches: the layers of one launch share one tile shape
GROUPS = [
    ("group 64x64 two layers", 64064, [Case("group conv 64x64", "group", 3, (3, 5, 7), 64, 64, 1, variant=64064, ragged=64),
                                       Case("group linear 64x64", "group", 9859, (1, 1, 1), 256, 256, 1, variant=64064, ragged=64, linear=True)]),
    ("group 128x128", 128128, [Case("group conv 128x128", "group", 2, WIDE, 256, 256, 1, variant=128128, ragged=128)]),
    ("group 128x64", 128064, [Case("group conv 128x64", "group", 2, (15, 21, 23), 256, 256, 1, variant=128064, ragged=128)]),
    ("group 64x128", 64128, [Case("group conv 64x128", "group", 2, (15, 21, 23), 64, 64, 3, variant=64128, ragged=64)]),
]

# csrc/conv_halo.hip (dreg_conv3_halo_n: 256 output channels on 4 x 8 x 8 boxes, 64 on 8 x 8 x 8; forward and the flipped-tap data-gradient pack)
# and csrc/conv_brick.hip (dreg_conv3_brick on the tiles of a flag volume) on the same generator and references; two boxes along every axis
# the kernel tiles, so box seams and all six faces are inside the comparison
HALO = [
    Case("halo fwd 256 bias up2 addend", "halo", 2, (8, 16, 24), 64, 256, 3, bias=True, addend="up2", amp=4),
    Case("halo fwd 64 bias same addend", "halo", 1, (16, 16, 24), 64, 64, 3, bias=True, addend="same", amp=4),
    Case("halo dgrad 256", "halo_dgrad", 2, (8, 16, 24), 256, 64, 3, amp=4),
    Case("halo dgrad 64", "halo_dgrad", 1, (16, 16, 24), 64, 128, 3),
]
BRICK = [
    Case("brick fwd 64 bias up2 addend", "brick", 2, (16, 16, 16), 64, 64, 3, nrows=3000, bias=True, addend="up2", amp=4),
    Case("brick fwd 256", "brick", 2, (16, 16, 16), 64, 256, 3, nrows=3000, amp=4),
]

ALL = FWD + DGRAD + WGRAD + [c for _, _, cs in GROUPS for c in cs]
assert len({c.name for c in ALL}) == len(ALL)
