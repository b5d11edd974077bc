"""The planted field and the input sets of the exact backward tests (tests/test_render_bwd_host.py on the CPU,
tests/test_hip_render_bwd_fp64.py on the GPU), the same objects for both.

The field is FLAT: every entry of level l holds the same fp16 pair (v[l][0], v[l][1]), multiples of 1/16 in [-1, 1], all 32 distinct and
non-zero.  The trilinear weights sum to 1 within ~1e-6, so the interpolated feature rounds to v in fp16 at every point: the encoding is one
constant vector.  The weights are sparse and dyadic (+-1, +-1/2, the last layer also +-1/4), so every activation of both nets is exact in
fp32 and representable in fp16, and the 16 SH columns of colour W1 are zero: sigma is one constant inside the model aabb, the colour one
fp16 triple, and a ray's survivors are the kept set tests/march_restatement.py decides.  Two densities, chosen through one weight of the
density net's output row: h0 = 1.4375 (alpha ~ 0.03 at dt 0.02: no ray ends early) and h0 = 3.875 (alpha ~ 0.3: most rays reach
T_all < 1e-4)."""
import functools
import math

import numpy as np

import march_cases as C
import render_bwd_restatement as RB
from oracle import ngp_oracle as N

DT = 0.02
H0 = {"thin": 1.4375, "dense": 3.875}
BKGD = C.BKGD
EDGE_COUNTS = (1, 63, 64, 65, 129)
WIDE_RAYS = 131073
WIDE_HITS = (63, 64, 127, 128, WIDE_RAYS - 1)
SET_RAYS = 2000


def levels():
    return RB.levels_of(N.level_table()[0])


def alpha64(h0, dt=DT):
    return 1.0 - math.exp(-math.exp(h0 - 1.0) * float(np.float32(dt)))


def _sparse(rng, rows, cols, per_row, values, col_lo=0):
    w = np.zeros((rows, cols))
    for i in range(rows):
        k = rng.choice(np.arange(col_lo, cols), per_row, replace=False)
        w[i, k] = rng.choice(values, per_row)
    return w


def _forward(v, d1, d2, c1, c2, c3):
    hd_pre = d1 @ v
    hd = np.maximum(hd_pre, 0.0)
    raw = d2 @ hd
    xin = np.concatenate([np.zeros(16), raw[1:16], [1.0]])
    h1_pre = c1 @ xin
    h1 = np.maximum(h1_pre, 0.0)
    h2_pre = c2 @ h1
    h2 = np.maximum(h2_pre, 0.0)
    o = c3 @ h2
    return dict(hd_pre=hd_pre, hd=hd, raw=raw, xin=xin, h1_pre=h1_pre, h1=h1, h2_pre=h2_pre, h2=h2, o=o)


def f16_boundary_distance(x):
    """Distance of x (fp64) to the nearest fp16 rounding boundary (the midpoint of two neighbouring fp16 values)."""
    h = np.float16(x)
    lo, hi = np.nextafter(h, np.float16(-np.inf)), np.nextafter(h, np.float16(np.inf))
    return np.minimum(np.abs(x - (np.float64(h) + np.float64(lo)) / 2), np.abs(x - (np.float64(h) + np.float64(hi)) / 2))


@functools.lru_cache(maxsize=None)
def planted(density):
    """dict: base / color (fp32 parameter vectors), weights (the five matrices, fp64), v [16,2], fwd (the constant forward record, fp64
    values that are exact fp16), h0, c (fp16 colour triple as fp64)."""
    halves, quarters = np.array([1.0, -1.0, 0.5, -0.5]), np.array([1.0, -1.0, 0.5, -0.5, 0.25, -0.25])
    for seed in range(20000):
        rng = np.random.default_rng(seed)
        vals = np.concatenate([np.arange(1, 17), -np.arange(1, 17)]) / 16.0
        v = rng.permutation(vals)
        d1 = _sparse(rng, 64, 32, 4, halves)
        d1[0] = 0.0
        d1[0, int(np.argmax(v == 0.5))] = 1.0                           # unit 0 holds exactly 1/2: the handle on h0
        d2 = _sparse(rng, 16, 64, 6, halves, col_lo=1)
        d2[0] = 0.0
        d2[0, rng.choice(np.arange(1, 64), 8, replace=False)] = rng.choice(halves, 8)
        c1 = _sparse(rng, 64, 32, 2, halves, col_lo=16)
        c1[:, 31] = rng.choice([0.5, -0.5, 0.25, -0.25, 1.0], 64)
        c2 = _sparse(rng, 64, 64, 3, halves)
        c3 = _sparse(rng, 16, 64, 6, quarters)
        f = _forward(v, d1, d2, c1, c2, c3)
        d2[0, 0] = 2.0 * (H0[density] - f["raw"][0])
        f = _forward(v, d1, d2, c1, c2, c3)
        pre = np.concatenate([f["hd_pre"], f["h1_pre"], f["h2_pre"]])
        ok = all(0.25 <= (f[k] > 0).mean() <= 0.75 for k in ("hd", "h1", "h2"))
        ok = ok and bool(np.all((pre == 0) | (np.abs(pre) >= 1.0 / 64)))
        o = f["o"][:3]
        ok = ok and len(set(o.tolist())) == 3 and bool(np.all(np.abs(o) <= 2.0)) and f["raw"][0] == H0[density]
        sig = 1.0 / (1.0 + np.exp(-o))
        ok = ok and bool(np.all(f16_boundary_distance(sig) >= 8 * 2.0 ** -24))
        everything = np.concatenate([f[k] for k in ("hd", "raw", "xin", "h1", "h2", "o")] + [d1.ravel(), d2.ravel(), c1.ravel(), c2.ravel(), c3.ravel()])
        ok = ok and bool(np.all(everything.astype(np.float16).astype(np.float64) == everything))
        # every table level must matter: a gradient on the three colour channels and on h0 reaches all 32 columns of the encoding
        r2 = (np.abs(c3[:3]).sum(0)) * (f["h2"] > 0)
        r1 = (np.abs(c2).T @ r2) * (f["h1"] > 0)
        rout = np.concatenate([[1.0], np.abs(c1[:, 16:31]).T @ r1])
        ok = ok and bool(np.all(rout > 0)) and bool(np.all(np.abs(d1).T @ ((np.abs(d2).T @ rout) * (f["hd"] > 0)) > 0))
        if ok:
            break
    else:
        raise AssertionError("no planted field found")
    rows, entries = N.level_table()
    table = np.zeros((entries, 2), np.float32)
    for l, r in enumerate(rows):
        table[r["offset"]:r["offset"] + r["size"]] = v[2 * l:2 * l + 2]
    base = np.concatenate([d1.ravel(), d2.ravel(), table.ravel()]).astype(np.float32)
    color = np.concatenate([c1.ravel(), c2.ravel(), c3.ravel()]).astype(np.float32)
    c = np.float16(1.0 / (1.0 + np.exp(-f["o"][:3]))).astype(np.float64)
    f["enc"] = v.copy()
    return dict(base=base, color=color, weights=dict(d1=d1, d2=d2, c1=c1, c2=c2, c3=c3), v=v.reshape(16, 2), fwd=f, h0=H0[density], c=c, seed=seed)


def sh16(d):
    """fp16 SH4 of the directions (the colour net's first 16 inputs), as fp64 values: oracle.ngp_oracle.sh4 in fp32, rounded to fp16."""
    import torch
    return N.sh4(torch.from_numpy(np.asarray(d, np.float32))).half().double().numpy()


def record_of(p, case, marched):
    """The flat regime's record for the kept samples of `marched`: broadcast constants, the SH columns per ray, the fp32 positions."""
    f = p["fwd"]
    xin = np.tile(f["xin"], (len(marched.n_idx), 1))
    xin[:, :16] = sh16(case.d)[marched.ray]
    return dict(enc=f["enc"][None], hd=f["hd"][None], raw=f["raw"][None], xin=xin, h1=f["h1"][None], h2=f["h2"][None], c=p["c"][None],
                x=RB.sample_positions(case.o, case.d, case.tmin32(), marched, case.dt))


# ------------------------------------------------------------------------------------------------------------------------ input sets
def _take(case, idx, name):
    return C.Case(name, case.binary, case.roi, case.scene, case.model, case.o[idx], case.d[idx], case.dt, jitter=case.jitter[idx])


@functools.lru_cache(maxsize=None)
def planted_set(jitter):
    """SET_RAYS rays of the ragged grid's training set at dt 0.02 (march_cases.random_case("ragged", 0.02, jitter): three distinct aabbs, the
    model aabb strictly inside the roi), all three ray families mixed."""
    full = C.random_case("ragged", DT, jitter)
    idx = np.sort(np.random.default_rng(31).permutation(len(full.o))[:SET_RAYS])
    return _take(full, idx, f"bwd-ragged-jitter{jitter}")


EDGE_LANES = (0, 62, 63, 64, 127, 128)        # with ray n - 1: the rays at the ends of a wave's 64 lanes and of a chunk, which must carry gradient


def _good(case):
    """Rays that are decidable and keep at least five samples inside the model aabb: a gradient flows through them."""
    return np.nonzero(case.ref.decidable & (case.ref.n_model >= 5))[0]


@functools.lru_cache(maxsize=None)
def edge_set(n):
    """n rays of planted_set("random"): consecutive ones (hits, misses and rays that stay outside the model aabb, as they come), with rays
    that carry gradient (_good) put at the lane and chunk edges EDGE_LANES and at ray n - 1."""
    full = planted_set("random")
    good = _good(full)
    idx = np.arange(int(good[0]), int(good[0]) + n)
    spare = [g for g in good.tolist() if g >= idx[-1] + 1]
    for k, pos in enumerate(sorted({p for p in EDGE_LANES + (n - 1,) if p < n})):
        idx[pos] = spare[k]
    return _take(full, idx, f"bwd-edge-{n}")


@functools.lru_cache(maxsize=None)
def wide_set():
    """131,073 rays (the first count at which a chunk of the backward holds 128 rays): all miss the scene aabb but the rays of
    planted_set("random"), which sit at 63, 64, 127, 128, the last index (rays that carry gradient: _good) and at random places between."""
    src = planted_set("random")
    rng = np.random.default_rng(41)
    where = np.array(WIDE_HITS)
    rest = np.setdiff1d(rng.permutation(WIDE_RAYS)[:SET_RAYS + 8], where)[:SET_RAYS - len(where)]
    where = np.sort(np.concatenate([where, rest]))
    order = np.arange(SET_RAYS)                                   # source ray of where[k]; a good ray is swapped into every rank of WIDE_HITS
    good = [g for g in _good(src).tolist()]
    ranks = np.searchsorted(where, np.array(WIDE_HITS))
    for k, rk in enumerate(ranks):
        j = int(np.nonzero(order == good[3 * k + 7])[0][0])
        order[rk], order[j] = order[j], order[rk]
    o = np.tile(np.array([[3.0, 2.5, -2.75]], np.float32), (WIDE_RAYS, 1)) + rng.random((WIDE_RAYS, 3)).astype(np.float32)
    d = np.tile(np.array([[0.6, 0.64, -0.48]], np.float32), (WIDE_RAYS, 1))                # away from the block: no ray meets the scene aabb
    jit = rng.random(WIDE_RAYS).astype(np.float32)
    o[where], d[where], jit[where] = src.o[order], src.d[order], src.jitter[order]
    case = C.Case("bwd-wide", src.binary, src.roi, src.scene, src.model, o, d, src.dt, jitter=jit)
    case.where = where
    return case


@functools.lru_cache(maxsize=None)
def miss_set(n=200):
    w = wide_set()
    idx = np.setdiff1d(np.arange(4000), w.where)[:n]
    return _take(w, idx, "bwd-all-miss")


def g_rgb_of(case, seed=17):
    return np.random.default_rng(seed).standard_normal((len(case.o), 3)).astype(np.float32)
