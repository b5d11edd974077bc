"""fp64 restatement of the ray march over a NeRF block's occupancy grid, written from the rule in the header of csrc/render.hip and
stepping EVERY lattice point one by one (no cell skipping, no coarse bits): the reference of tests/test_hip_march_exact.py.

For a ray with origin o and direction d (used as given, not normalised):
  interval   slab test against the scene aabb; an axis with d[k] == 0 keeps the slab iff lo <= o[k] <= hi.  near = max of the entry
             parameters, far = min of the exit parameters, hit = near <= far and far > 0.  t_min = max(near, 0, near_plane) + jitter dt,
             t_max = min(far, far_plane); the visibility form has no planes and t_max = |point - camera| (not clipped by far)
  lattice    t_mid = t_min + (n + 1/2) dt for n = 0, 1, ... while t_mid < t_max
  kept       x = o + t_mid d lies in the roi aabb (0 <= u <= 1 on every axis, u = (x - lo) / ext) and its cell floor(u res), clamped to the
             grid, is set
  in_model   x lies strictly inside the model aabb (outside: sigma = 0 — the sample is still kept and counted)

Inputs are fp32 values (the arrays the kernels receive); all arithmetic here is fp64, which represents them and every lattice index exactly.

Decidability.  The kernels evaluate the same rule in fp32, so a ray's kept set can differ from this one only where a rounding can move a
sample across a decision.  With u = 2^-24 (half an fp32 ulp, relative), the fp32 position of lattice sample n on axis k is
  x_k = fl(o_k + fl(t d_k)),  t = fl(t_min + fl((n + 1/2) dt)),  t_min = fl(fl(lo - o) fl(1 / d))                      (render_ray_interval)
  |error of t_min| <= 3u t_min;  |error of t| <= 3u t_min + u (t - t_min) + u t <= 4u t;  |error of t d_k| <= 5u t |d_k|;
  |error of x_k| <= u (5 t |d_k| + |x_k|) <= u (|o_k| + 6 t |d_k|)
and the cell index floor(fl(fl(fl(x_k - lo_k) / fl(hi_k - lo_k)) res_k)) adds four more roundings of a quantity <= ext_k: 4u ext_k in
position.  A direction that the kernel itself forms in fp32 (the visibility rays: d = fl(fl(p - c) fl(1 / fl(sqrt(sum of squares)))), five
roundings) adds dir_err = 5 to the coefficient of t |d_k|.  The position margin of a sample on axis k is twice that bound:
  margin_k = 2 * 2^-24 * (|o_k| + (6 + dir_err) t |d_k| + 4 ext_k)                                   ("a small multiple of 2^-24 (|o| + t |d|)")
and a quantity in t (the interval's ends, a lattice point against t_max) gets margin_t = 2 * 2^-24 * (4 t + 3 t_max + 3 |t_min|): the
position bound converted to t through the ray's direction, i.e. the relative roundings of the quotients (lo - o) / d.
A ray is UNDECIDABLE when
  * a lattice sample lies within margin_k of a cell face on some axis and the cells it could fall into instead (any combination of the near
    axes; beyond the roi = unoccupied) do not all share its occupancy,
  * a kept (or possibly kept) sample lies within margin_k of a face plane of the model aabb,
  * t_max lies within margin_t of a lattice point, or
  * the slab test is within margin_t of the other answer (near against far) AND that margin reaches dt / 2: below it the interval of either
    answer is too short to hold a lattice point, so the kept set is empty both ways (Marched.hit_sure still says which rays these are).
"""
import numpy as np

U = 2.0 ** -24
_CHUNK_SAMPLES = 1 << 20


def interval(o, d, scene, near_plane=None, far_plane=None):
    """(t_min, t_max, hit, margin-free near/far) in fp64 for rays o, d [R,3]: the slab rule of the module docstring, before jitter."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    lo, hi = np.asarray(scene[:3], np.float64), np.asarray(scene[3:], np.float64)
    par = d == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / np.where(par, 1.0, d), (hi - o) / np.where(par, 1.0, d)
    tlo = np.where(par, -np.inf, np.minimum(t0, t1))
    thi = np.where(par, np.inf, np.maximum(t0, t1))
    near, far = tlo.max(axis=1), thi.min(axis=1)
    in_slab = ((o >= lo) & (o <= hi)) | ~par
    hit = in_slab.all(axis=1) & (near <= far) & (far > 0)
    tmin = np.maximum(near, 0.0)
    tmax = far.copy()
    if near_plane is not None:
        tmin = np.maximum(tmin, float(near_plane))
    if far_plane is not None:
        tmax = np.minimum(tmax, float(far_plane))
    return tmin, tmax, hit, near, far


class Marched:
    """Per-ray results in CSR form: ray r's kept samples are [ptr[r], ptr[r + 1]) of n_idx (lattice index), t_mid, in_model."""

    def __init__(self, ptr, n_idx, t_mid, in_model, hit, decidable, t_min, t_max, hit_sure):
        self.ptr, self.n_idx, self.t_mid, self.in_model = ptr, n_idx, t_mid, in_model
        self.hit, self.decidable, self.t_min, self.t_max, self.hit_sure = hit, decidable, t_min, t_max, hit_sure
        self.n_kept = np.diff(ptr)
        self.ray = np.repeat(np.arange(len(ptr) - 1), self.n_kept)
        self.n_model = np.bincount(self.ray, weights=in_model, minlength=len(ptr) - 1).astype(np.int64)

    def kept(self, r):
        s = slice(self.ptr[r], self.ptr[r + 1])
        return self.n_idx[s], self.t_mid[s], self.in_model[s]

    def rank(self):
        """For every kept sample: the number of in-model kept samples before it on its ray."""
        cm = np.cumsum(self.in_model) - self.in_model
        base = np.zeros(len(self.ptr) - 1, np.int64)
        some = self.n_kept > 0
        base[some] = cm[self.ptr[:-1][some]]
        return cm - base[self.ray]

    def composite(self, a, q=None):
        """The closed form of a field with constant alpha `a` inside the model aabb and 0 outside it: (opacity, depth) per ray, fp64.
        w = a q^j for the j-th in-model kept sample, q = 1 - a unless given (the kernel's own fp32 value of 1 - a)."""
        q = 1.0 - a if q is None else q
        R = len(self.ptr) - 1
        w = np.where(self.in_model, a * q ** self.rank(), 0.0)
        return np.bincount(self.ray, weights=w, minlength=R), np.bincount(self.ray, weights=w * self.t_mid, minlength=R)


def march(o, d, binary, roi, scene, model, dt, near_plane=None, far_plane=None, jitter=None, t_max=None, dir_err=0.0, exact=False):
    """March rays o, d [R,3] (fp32 values).  binary: bool [rx,ry,rz]; roi / scene / model: 6 floats each; dt: the step (rounded to fp32, as
    the kernels receive it); jitter: optional [R] in [0,1); t_max: optional [R], replaces min(far, far_plane) (the visibility form);
    exact: the caller's inputs make every fp32 operation exact (dyadic values), so no rounding exists and every ray is decidable.
    Returns a Marched."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    binary = np.asarray(binary).astype(bool)
    res = np.array(binary.shape, np.int64)
    roi, scene, model = (np.asarray(np.asarray(v, np.float32), np.float64) for v in (roi, scene, model))
    dt = float(np.float32(dt))
    R = o.shape[0]
    tmin, tmax, hit, near, far = interval(o, d, scene, near_plane, far_plane)
    if t_max is not None:
        tmax = np.asarray(t_max, np.float64).copy()
        hit = hit & (tmax > 0)
    if jitter is not None:
        tmin = tmin + np.asarray(np.asarray(jitter, np.float32), np.float64) * dt
    tmin = np.where(hit, tmin, 0.0)
    tmax = np.where(hit, tmax, 0.0)
    # lattice points with t_mid < t_max: n < (t_max - t_min) / dt - 1/2
    cnt = np.where(hit & (tmin < tmax), np.ceil((tmax - tmin) / dt - 0.5), 0).astype(np.int64).clip(min=0)
    mt_ray = 2 * U * (7 * np.abs(tmax) + 3 * np.abs(tmin))
    decidable = np.ones(R, bool)
    fin = np.isfinite(near) & np.isfinite(far)
    with np.errstate(invalid="ignore"):
        # hit against miss: near within margin of far.  Either answer leaves an interval shorter than the margin, which holds no lattice point
        # (the first one sits at t_min + dt / 2) unless the margin reaches dt / 2; far against 0 is a sign, which no rounding changes.
        mt_slab = 2 * U * 3 * (np.abs(near) + np.abs(far))
        hit_sure = ~(fin & (np.abs(far - near) <= mt_slab))
    decidable &= hit_sure | (mt_slab < 0.5 * dt)
    roi_lo, ext = roi[:3], roi[3:] - roi[:3]
    cell = ext / res
    out_ptr, out_n, out_t, out_m = [0], [], [], []
    r0 = 0
    while r0 < R:
        r1, tot = r0, 0
        while r1 < R and (r1 == r0 or tot + cnt[r1] <= _CHUNK_SAMPLES):
            tot += cnt[r1]
            r1 += 1
        c = cnt[r0:r1]
        ray = np.repeat(np.arange(r0, r1), c)
        n = np.arange(tot) - np.repeat(np.cumsum(c) - c, c)
        t = tmin[ray] + (n + 0.5) * dt
        x = o[ray] + t[:, None] * d[ray]
        margin = 2 * U * (np.abs(o[ray]) + (6 + dir_err) * t[:, None] * np.abs(d[ray]) + 4 * ext)
        uu = (x - roi_lo) / ext
        g = uu * res
        i = np.floor(g).astype(np.int64)
        i = np.where(uu == 1.0, res - 1, i)                         # the roi's upper face belongs to the last cell (floor + clamp)
        inside = ((uu >= 0) & (uu <= 1)).all(axis=1)

        def lookup(idx):
            ok = ((idx >= 0) & (idx < res)).all(axis=1)
            j = idx.clip(0, res - 1)
            return binary[j[:, 0], j[:, 1], j[:, 2]] & ok

        occ = lookup(i) & inside
        # cells the fp32 evaluation could choose instead
        lo_gap, hi_gap = (g - i) * cell, (i + 1 - g) * cell
        step = np.where(lo_gap <= margin, -1, 0) + np.where(hi_gap <= margin, 1, 0)      # (margin << cell: never both)
        near_any = (step != 0).any(axis=1)
        ambiguous = np.zeros(tot, bool)
        anyocc = occ.copy()
        if near_any.any():
            sel = np.nonzero(near_any)[0]
            for s in range(1, 8):
                bits = np.array([(s >> k) & 1 for k in range(3)])
                alt = lookup(i[sel] + step[sel] * bits)
                ambiguous[sel] |= alt != occ[sel]
                anyocc[sel] |= alt
        mlo, mhi = model[:3], model[3:]
        near_model = ((np.abs(x - mlo) <= margin) | (np.abs(x - mhi) <= margin)).any(axis=1)
        bad = ambiguous | (near_model & anyocc)
        if bad.any():
            decidable[np.unique(ray[bad])] = False
        in_model = ((x > mlo) & (x < mhi)).all(axis=1)
        keep = occ
        out_n.append(n[keep]); out_t.append(t[keep]); out_m.append(in_model[keep])
        per = np.bincount(ray[keep] - r0, minlength=r1 - r0)
        out_ptr.extend((out_ptr[-1] + np.cumsum(per)).tolist())
        r0 = r1
    # t_max against the last lattice point before it and the first one beyond it (an interval within margin of empty keeps nothing either
    # way: its first lattice point sits at t_min + dt / 2)
    last_gap = np.minimum(np.abs(tmin + (cnt - 0.5) * dt - tmax), np.abs(tmin + (cnt + 0.5) * dt - tmax))
    decidable &= ~(hit & (tmin < tmax) & (last_gap <= mt_ray))
    if exact:
        decidable[:] = True
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return Marched(np.asarray(out_ptr, np.int64), cat(out_n, np.int64), cat(out_t, np.float64), cat(out_m, bool), hit, decidable, tmin, tmax, hit_sure)


def visibility(cams, pts, binary, roi, scene, model, dt):
    """The visibility form: every (camera, point) ray starts at the camera, points at the point, t_max = their distance; a ray SEES the
    surface when it keeps an in-model sample (cut_off = alpha / 2, alpha_thre = 0: the first such sample decides).  Returns (label [Np] bool,
    decidable [Np] bool, per-ray Marched with rays ordered camera-major): a point is decidable when all its rays are, or a decidable ray sees."""
    cams, pts = np.asarray(cams, np.float64).reshape(-1, 3), np.asarray(pts, np.float64).reshape(-1, 3)
    Nc, Np = cams.shape[0], pts.shape[0]
    o = np.repeat(cams, Np, axis=0)
    diff = np.tile(pts, (Nc, 1)) - o
    dist = np.sqrt((diff * diff).sum(axis=1))
    d = diff / np.where(dist > 0, dist, 1.0)[:, None]
    m = march(o, d, binary, roi, scene, model, dt, t_max=dist, dir_err=5.0)
    sees = (m.n_model > 0).reshape(Nc, Np)
    dec = m.decidable.reshape(Nc, Np)
    label = sees.any(axis=0)
    decidable = dec.all(axis=0) | (sees & dec).any(axis=0)
    return label, decidable, m
