"""The input sets of the exact march tests (tests/test_march_host.py on the CPU, tests/test_hip_march_exact.py on the GPU): grids, aabbs and
rays as fp32 numpy arrays, the same objects for both files, with the fp64 reference (tests/march_restatement.py) of each computed once.

The field of these tests has a zeroed hash table: sigma = exp(-1) at every sample strictly inside the model aabb, so a sample's alpha is the
constant a = 1 - exp(-exp(-1) dt) and a rendered ray is a closed form of the set of samples it kept (Marched.composite)."""
import functools
import math

import numpy as np

import march_restatement as MR

BKGD = (0.25, 0.5, 1.0)


def alpha64(dt):
    return 1.0 - math.exp(-math.exp(-1.0) * float(np.float32(dt)))


def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


class Case:
    """One launch: grid, three aabbs, rays, step and planes; .ref is the fp64 march (cached)."""

    def __init__(self, name, binary, roi, scene, model, o, d, dt, near=None, far=None, jitter=None, exact=False, family=None):
        self.name, self.binary = name, np.ascontiguousarray(binary.astype(bool))
        self.roi, self.scene, self.model = ([float(np.float32(v)) for v in a] for a in (roi, scene, model))
        self.o, self.d, self.dt, self.near, self.far = f32(o), f32(d), float(np.float32(dt)), near, far
        self.jitter = None if jitter is None else f32(jitter)
        self.exact, self.family = exact, family
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = MR.march(self.o, self.d, self.binary, self.roi, self.scene, self.model, self.dt, self.near, self.far, self.jitter, exact=self.exact)
        return self._ref

    def tmin32(self):
        """t_min as fp32 arithmetic gives it (the slab rule with a rounded reciprocal, then planes and jitter): the closed form's fp32 run."""
        o, d = self.o, self.d
        lo, hi = np.float32(self.scene[:3]), np.float32(self.scene[3:])
        par = d == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = (np.float32(1) / np.where(par, np.float32(1), d)).astype(np.float32)
            t0, t1 = ((lo - o) * inv).astype(np.float32), ((hi - o) * inv).astype(np.float32)
        near = np.where(par, np.float32(-1e30), np.minimum(t0, t1)).max(axis=1)
        tmin = np.maximum(near, np.float32(0))
        if self.near is not None:
            tmin = np.maximum(tmin, np.float32(self.near))
        if self.jitter is not None:
            tmin = (tmin + (self.jitter * np.float32(self.dt)).astype(np.float32)).astype(np.float32)
        return tmin.astype(np.float32)

    def stepped_fp32(self):
        """The rule of tests/march_restatement.py evaluated in fp32, one rounding per operation, at EVERY lattice point: t = fl(t_min + fl((n + 1/2)
        dt)), x = fl(o + fl(t d)), u = fl(fl(x - lo) / fl(hi - lo)), cell = floor(fl(u res)) clamped.  Returns (kept samples, kept samples inside
        the model aabb) per ray.  A marcher that works in fp32 without fused multiply-adds and with correctly rounded division returns exactly
        these samples on EVERY ray, decidable or not — whatever it passes over in between."""
        f = np.float32
        o, d, dt = self.o, self.d, f(self.dt)
        lo, hi = f(self.scene[:3]), f(self.scene[3:])
        par = d == 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = f(1) / np.where(par, f(1), d)
            t0, t1 = (lo - o) * inv, (hi - o) * inv
        near = np.where(par, f(-1e30), np.minimum(t0, t1)).max(axis=1)
        far = np.where(par, f(1e30), np.maximum(t0, t1)).min(axis=1)
        hit = (((o >= lo) & (o <= hi)) | ~par).all(axis=1) & (near <= far) & (far > 0)
        tmin, tmax = self.tmin32(), far if self.far is None else np.minimum(far, f(self.far))
        rlo, rext, res = f(self.roi[:3]), f(self.roi[3:]) - f(self.roi[:3]), np.array(self.binary.shape)
        mlo, mext = f(self.model[:3]), f(self.model[3:]) - f(self.model[:3])
        live = hit & (tmin < tmax)
        cnt = np.where(live, np.ceil((tmax.astype(np.float64) - tmin) / float(dt)) + 2, 0).astype(np.int64)
        kept, model = np.zeros(len(o), np.int64), np.zeros(len(o), np.int64)
        r0 = 0
        while r0 < len(o):
            r1 = r0 + max(1, int(np.searchsorted(np.cumsum(cnt[r0:]), 1 << 21)))
            c = cnt[r0:r1]
            ray = np.repeat(np.arange(r0, r1), c)
            n = (np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)).astype(f)
            tm = tmin[ray] + (n + f(0.5)) * dt
            x = o[ray] + tm[:, None] * d[ray]
            u = (x - rlo) / rext
            ci = np.clip(np.floor(u * res.astype(f)).astype(np.int64), 0, res - 1)
            occ = self.binary[ci[:, 0], ci[:, 1], ci[:, 2]] & ((u >= 0) & (u <= 1)).all(axis=1) & (tm < tmax[ray])
            um = (x - mlo) / mext
            kept[r0:r1] = np.bincount(ray[occ] - r0, minlength=r1 - r0)
            model[r0:r1] = np.bincount(ray[occ & ((um > 0) & (um < 1)).all(axis=1)] - r0, minlength=r1 - r0)
            r0 = r1
        return kept, model

    def depth_fp32_error(self, a=None):
        """max over the rays of |closed form accumulated in fp32, in the kernel's order - fp64 closed form|, and the fp64 depth: the rounding
        the depth tolerance has to cover (tolerance = 4 x this)."""
        r = self.ref
        a32 = np.float32(alpha64(self.dt) if a is None else a)
        q32 = np.float32(1) - a32
        _, dep64 = r.composite(float(a32), float(q32))
        R = len(r.n_kept)
        tmin = self.tmin32()
        Ts, dep = np.ones(R, np.float32), np.zeros(R, np.float32)
        rank = r.rank()
        dt32 = np.float32(self.dt)
        for j in range(int(r.n_model.max()) if R and len(rank) else 0):
            sel = np.nonzero(r.in_model & (rank == j))[0]
            ray = r.ray[sel]
            tm = (tmin[ray] + ((r.n_idx[sel].astype(np.float32) + np.float32(0.5)) * dt32).astype(np.float32)).astype(np.float32)
            w = (a32 * Ts[ray]).astype(np.float32)
            Ts[ray] = (Ts[ray] * q32).astype(np.float32)
            dep[ray] = (dep[ray] + (w * tm).astype(np.float32)).astype(np.float32)
        return float(np.abs(dep.astype(np.float64) - dep64).max()) if R else 0.0, dep64

    def depth_tolerance(self, a=None):
        """4 x depth_fp32_error at alpha `a` (the GPU test passes the kernel's own alpha, the one its closed form uses: the roundings of T *= q
        depend on the bits of q, so the difference at the fp64 alpha rounded to fp32 says nothing about another alpha a few ulps away)."""
        return 4.0 * self.depth_fp32_error(a)[0]

    def step_sensitivity(self):
        """Per ray: a (1 - a)^n dt, a lower bound of the change of depth when any one of its n kept in-model samples moves by one lattice step."""
        a = alpha64(self.dt)
        return a * (1.0 - a) ** self.ref.n_model * self.dt


# ------------------------------------------------------------------------------------------------------------------------ exact cases
EXACT_GRIDS = {"cube8": ((8, 8, 8), [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]), "slab8x4x16": ((8, 4, 16), [-1.0, -0.5, -2.0, 1.0, 0.5, 2.0])}
EXACT_PLANES = {"open": (None, None), "faces": (1.0 / 128, None), "near_beyond_far": (0.5, 0.25)}
EXACT_PATTERNS = ("full", "empty", "single", "checker", "last_x", "last_y", "last_z")
EXACT_MODEL = [-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]
EXACT_DT = 1.0 / 64


def exact_pattern(shape, name):
    b = np.zeros(shape, bool)
    rx, ry, rz = shape
    if name == "full":
        b[:] = True
    elif name == "single":
        b[3, 1, 5] = True
    elif name == "checker":
        i, j, k = np.meshgrid(np.arange(rx), np.arange(ry), np.arange(rz), indexing="ij")
        b = (i + j + k) % 2 == 0
    elif name == "last_x":
        b[rx - 1, 1, 2] = True
    elif name == "last_y":
        b[2, ry - 1, 1] = True
    elif name == "last_z":
        b[1, 2, rz - 1] = True
    return b


def exact_rays(aabb):
    """Origins on a 1/16 lattice — outside, on a face, just inside, on an inner cell face, inside, on the far face, beyond — crossed with the six
    axis directions (zeros of either sign) and dyadic diagonals.  Includes rays in a boundary plane (o[k] == lo, d[k] == 0), rays pointing away,
    and, with a near plane of 1/128, samples exactly on cell faces."""
    lo, hi = np.array(aabb[:3]), np.array(aabb[3:])
    per_axis = [np.array([l - 0.5, l, l + 1 / 16, l + (h - l) / 2, h - 5 / 16, h, h + 0.5]) for l, h in zip(lo, hi)]
    O = np.stack(np.meshgrid(*per_axis, indexing="ij"), -1).reshape(-1, 3)
    dirs = []
    for k in range(3):
        for s in (1.0, -1.0):
            for z in (0.0, -0.0):
                v = np.full(3, z)
                v[k] = s
                dirs.append(v)
    dirs += [np.array(v) for v in ((1.0, 1.0, 0.0), (-1.0, 1.0, -0.0), (1.0, 0.5, -0.25), (-0.5, -1.0, 1.0), (0.0, 1.0, -1.0))]
    D = np.stack(dirs)
    o = np.repeat(O, len(D), axis=0)
    d = np.tile(D, (len(O), 1))
    return f32(o), f32(d)


@functools.lru_cache(maxsize=None)
def exact_case(grid, planes, pattern):
    shape, aabb = EXACT_GRIDS[grid]
    o, d = exact_rays(aabb)
    near, far = EXACT_PLANES[planes]
    return Case(f"exact-{grid}-{planes}-{pattern}", exact_pattern(shape, pattern), aabb, aabb, EXACT_MODEL, o, d, EXACT_DT, near, far, exact=True)


def calibration_case(dt=EXACT_DT):
    """One ray that keeps exactly one sample: along +x through the single occupied cell of an 8^3 grid, between planes one step apart."""
    b = np.zeros((8, 8, 8), bool)
    b[4, 4, 4] = True
    aabb = EXACT_GRIDS["cube8"][1]
    near = 2.0 + 1.0 / 16
    return Case(f"calibration-dt{dt}", b, aabb, aabb, EXACT_MODEL, [[-2.0, 0.125, 0.125]], [[1.0, 0.0, 0.0]], dt, near=near, far=float(np.float32(near + dt)))


# ------------------------------------------------------------------------------------------------------------- random and grazing cases
RANDOM_GRIDS = ("shell128", "ragged", "random10")
RANDOM_DTS = (0.02, 0.005, 1e-3)
SCALE = {0.02: 1.0, 0.005: 0.5, 1e-3: 0.125}        # the block shrinks with the step: n a <= 2 and a decodable n at every dt
RAYS_PER_FAMILY = 1500


def _grid(name):
    if name == "shell128":
        shape, half = (128, 128, 128), np.array([0.6, 0.6, 0.6])
        c = [(np.arange(n) + 0.5) / n * 2 - 1 for n in shape]
        X, Y, Z = np.meshgrid(*c, indexing="ij")
        rad = np.sqrt(X * X + Y * Y + Z * Z)
        b = (rad > 0.55) & (rad < 0.8)
    elif name in ("ragged", "ragged_cut"):
        shape, half = (30, 22, 37), np.array([0.6, 0.44, 0.74])
        c = [(np.arange(n) + 0.5) / n * 2 - 1 for n in shape]
        X, Y, Z = np.meshgrid(*c, indexing="ij")
        rad = np.sqrt(X * X + 0.8 * Y * Y + 1.2 * Z * Z)
        b = ((rad > 0.5) & (rad < 0.85)) | ((X > 0.8) & (Y > 0.7)) | (Z > 0.93)          # a shell plus pieces in the cut last blocks
        if name == "ragged_cut":
            b &= X + 0.3 * Y - 0.2 * Z > -0.1                                            # half of it cut away: some points see no surface
    else:
        shape, half = (40, 40, 40), np.array([0.6, 0.6, 0.6])
        b = np.random.default_rng(7).random(shape) < 0.10
    return b, half


def _aabbs(half, s):
    """Three distinct boxes: the scene larger than the roi, the model aabb smaller than it, none centred on another
    (no round numbers: an axis-parallel ray enters at the scene's face, and a face offset that is a multiple of dt would put its whole lattice
    on cell faces)"""
    roi = np.concatenate([-half + [0.0317, -0.0213, 0.0109], half + [0.0317, -0.0213, 0.0109]]) * s
    scene = roi + np.array([-0.1537, -0.1049, -0.2113, 0.1271, 0.1817, 0.1093]) * s
    model = roi + np.array([0.0713, 0.0529, 0.1131, -0.0917, -0.0611, -0.0433]) * s
    return roi, scene, model


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rays(roi, scene, s, rng, n):
    lo, hi = roi[:3], roi[3:]
    slo, shi = scene[:3], scene[3:]
    # generic: three eyes outside the scene looking at random points of the block
    eyes = np.array([[1.6, -1.1, 0.7], [-0.3, 1.5, -1.2], [-1.4, -0.4, 1.3]]) * s
    e = eyes[rng.integers(0, 3, n)]
    tgt = lo + rng.random((n, 3)) * (hi - lo) * 1.1 - 0.05 * (hi - lo)
    fam = [(e, _unit(tgt - e))]
    # grazing: nearly parallel to an axis, the two other components of order 1e-3 and smaller; they start outside the scene
    k = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    d = rng.uniform(-1, 1, (n, 3)) * 1e-3 * 10.0 ** (-rng.uniform(0, 3, (n, 3)))
    d[np.arange(n), k] = sign
    o = slo + rng.random((n, 3)) * (shi - slo)
    o[np.arange(n), k] = np.where(sign > 0, slo[k] - 0.3137 * s, shi[k] + 0.2871 * s)
    fam.append((o, _unit(d)))
    # inside: origins anywhere in the scene aabb (most of them inside the roi), directions over the sphere
    fam.append((slo + rng.random((n, 3)) * (shi - slo), _unit(rng.normal(size=(n, 3)))))
    return np.concatenate([f[0] for f in fam]), np.concatenate([f[1] for f in fam]), np.repeat(np.arange(3), n)


FAMILIES = ("generic", "grazing", "inside")


@functools.lru_cache(maxsize=None)
def random_case(grid, dt, jitter=None):
    """grid in RANDOM_GRIDS, dt in RANDOM_DTS; jitter: None, a float (every ray) or "random"."""
    b, half = _grid(grid)
    s = SCALE[dt]
    roi, scene, model = _aabbs(half, s)
    rng = np.random.default_rng(1000 * RANDOM_GRIDS.index(grid) + RANDOM_DTS.index(dt))
    o, d, fam = _rays(f32(roi).astype(np.float64), f32(scene).astype(np.float64), s, rng, RAYS_PER_FAMILY)
    jit = None
    if jitter == "random":
        jit = np.random.default_rng(5).random(len(o)).astype(np.float32)
    elif jitter is not None:
        jit = np.full(len(o), jitter, np.float32)
    return Case(f"{grid}-dt{dt}" + ("" if jitter is None else f"-jitter{jitter}"), b, roi, scene, model, o, d, dt, jitter=jit, family=fam)


JITTERS = (0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0))), "random")


def train_case(jitter):
    return random_case("ragged", 0.005, jitter)


def random_cases():
    return [random_case(g, dt) for g in RANDOM_GRIDS for dt in RANDOM_DTS]


# ---------------------------------------------------------------------------------------------------------------------------- coarse bits
STEPPED_SLICE = slice(6000, 9000)       # the rays of coarse_rays() that are also compared with Case.stepped_fp32 (a host copy of the old skip loses samples on ray 7217)


def coarse_rays(n=20000, seed=6):
    """Nearly axis-parallel rays through a 128^3 shell over [-1.5, 1.5]^3 at render_image's default step of 1e-3: the launch where skipping an
    empty 4^3 block is most exposed to the rounding of the block's exit (no reference is needed: both launches run the same fp32 arithmetic)."""
    rng = np.random.default_rng(seed)
    shape = (128, 128, 128)
    c = [(np.arange(m) + 0.5) / m * 3 - 1.5 for m in shape]
    X, Y, Z = np.meshgrid(*c, indexing="ij")
    rad = np.sqrt(X * X + Y * Y + Z * Z)
    b = (rad > 0.55) & (rad < 1.05)
    aabb = [-1.5] * 3 + [1.5] * 3
    k = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    d = rng.uniform(-1, 1, (n, 3)) * 1e-3 * 10.0 ** (-rng.uniform(0, 3, (n, 3)))
    d[np.arange(n), k] = sign
    o = rng.uniform(-1.5, 1.5, (n, 3))
    o[np.arange(n), k] = -2.0 * sign
    return b, aabb, f32(o), f32(_unit(d))


# ---------------------------------------------------------------------------------------------------------------------------- visibility
class VisCase:
    def __init__(self, name, binary, roi, scene, model, cams, pts, dt):
        self.name, self.binary = name, np.ascontiguousarray(binary.astype(bool))
        self.roi, self.scene, self.model = ([float(np.float32(v)) for v in a] for a in (roi, scene, model))
        self.cams, self.pts, self.dt = f32(cams), f32(pts), float(np.float32(dt))
        self._ref = None

    @property
    def ref(self):
        """(label [Np], decidable [Np], Marched of the Nc * Np rays)"""
        if self._ref is None:
            self._ref = MR.visibility(self.cams, self.pts, self.binary, self.roi, self.scene, self.model, self.dt)
        return self._ref

    @property
    def cut_off(self):
        return 0.5 * alpha64(self.dt)


@functools.lru_cache(maxsize=None)
def vis_case(distinct_aabbs=True):
    """Points on a lattice over the scene aabb plus random ones; cameras outside, inside and on a face of the scene aabb, all ON that lattice's
    lines, so that many camera-point rays have one or two direction components of exactly 0; one camera coincides with a point (t_max = 0)."""
    b, half = _grid("ragged_cut")
    roi, scene, model = _aabbs(half, 1.0)
    if not distinct_aabbs:
        scene = roi
    roi, scene, model = (f32(v).astype(np.float64) for v in (roi, scene, model))
    ax = [np.float32(scene[k]) + np.arange(m, dtype=np.float32) * np.float32((scene[3 + k] - scene[k]) / (m - 1)) for k, m in enumerate((11, 9, 12))]
    ax = [a.astype(np.float64) for a in ax]
    for k in range(3):
        ax[k][-1] = scene[3 + k]
    P = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(11)
    P = np.concatenate([P, scene[:3] + rng.random((600, 3)) * (scene[3:] - scene[:3])])
    cams = np.array([
        [ax[0][5], ax[1][4], scene[5] + 0.5],             # outside, above: looks down lattice lines (d = (0, 0, -1) for a column of points)
        [scene[0] - 0.625, ax[1][2], ax[2][7]],           # outside, along x
        [ax[0][5], ax[1][4], ax[2][6]],                   # inside the shell's hollow, ON a lattice point: t_max = 0 for that point
        [scene[3], ax[1][1], ax[2][9]],                   # on the scene aabb's +x face
        [1.3, -1.2, 0.9],                                 # outside, generic
    ])
    return VisCase("vis-ragged" + ("" if distinct_aabbs else "-one-aabb"), b, roi, scene, model, cams, P, 0.02)
