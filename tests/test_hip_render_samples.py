"""GPU: NeRF block training on a sample list (csrc/render_samples.hip).

1. The forward's bits: rgb, opacity, depth and the count of dreg_ngp_render_train_samples equal dreg_ngp_render_train's.
2. The list, in canonical order: its length, ord, x = fl(o + fl(t d)), the last record of a ray against the ray's outputs, and on the planted flat
   field (tests/render_bwd_cases.py) t and the kept set against the fp64 march (tests/march_restatement.py).
3. Capacity: 0, count - 1 and count through the raw entry point (per-ray outputs unchanged, the true count, sentinel bands untouched, the records
   written a subset of the full list), and the wrapper at sample_capacity = 1.
4. dreg_ngp_samples_grad against the fp64 rule of tests/render_samples_restatement.py on the kernel's own records, element by element, within
   (C + n) 2^-24 M: C the fp32 roundings counted from ngp_samples_grad_kernel, n the accumulated terms, M the sum of the absolute terms.
5. The whole backward against fp64 on the planted field, element by element, in the bound form of tests/test_hip_field_train.py with the
   sample-gradient kernel's (and the forward record's) roundings added to C; with g_rgb alone the reference is render_bwd_restatement.backward64.
6. A general field against CPU autograd with the three-term loss; determinism across runs and launch widths; opacity-only and depth-only
   losses reach the parameters; train_ngp_nerf.py --backward samples end to end."""
import functools
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import march_cases as C
import ngp_grad_restatement as GR
import render_bwd_cases as B
import render_bwd_restatement as RB
import render_samples_restatement as RS
import render_train_restatement as RT
import test_hip_render_bwd_fp64 as G

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
RECORD = ("ray", "ord", "t", "x", "T_next", "w", "c", "P", "Pd")
WIDTH = {"x": 3, "c": 3, "P": 3}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------------------ launches
BAND = 64                     # sentinel records behind every record array
SENT_F, SENT_I = -12345.5, -123456789


def _raw(dev, f, grid, o, d, jit, scene, dt, bkgd, capacity, alpha_thre=0.0):
    """dreg_ngp_render_train_samples through the C entry, record arrays of capacity + BAND rows with the band holding a sentinel:
    (rgb, opacity, depth, n_samples, true count, records [capacity rows], bands)."""
    from dreg_nerf_amd import lib as L, render as R
    lib = L.load()
    n = o.shape[0]
    roi, b8, bits = R._grid_parts(grid, dev)
    rgb = torch.empty(n, 3, device=dev)
    opacity, depth = torch.empty(n, device=dev), torch.empty(n, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    rec = {}
    for k in RECORD:
        isint = k in ("ray", "ord")
        shape = (capacity + BAND, WIDTH[k]) if k in WIDTH else (capacity + BAND,)
        rec[k] = torch.full(shape, SENT_I if isint else SENT_F, dtype=torch.int32 if isint else torch.float32, device=dev)
    f._prepared()
    L.check(lib.dreg_ngp_render_train_samples(L.ptr(o), L.ptr(d), L.ptr(jit), n, L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], L.ptr(bits),
                                              *f.density_ptrs(), *f.color_ptrs(), *f._levels, L.f6(roi), L.f6(scene), L.f6(f._aabb_host()),
                                              -math.inf, math.inf, float(dt), float(alpha_thre), 1e-4, L.f3(bkgd), L.ptr(rgb), L.ptr(opacity), L.ptr(depth),
                                              counters.data_ptr(), counters.data_ptr() + 8, capacity, *[L.ptr(rec[k]) for k in RECORD],
                                              counters.data_ptr() + 16, L.stream()), "dreg_ngp_render_train_samples")
    c = counters.cpu()
    assert int(c[1]) >= 0
    return rgb, opacity, depth, int(c[0]), int(c[2]), {k: v[:capacity] for k, v in rec.items()}, {k: v[capacity:] for k, v in rec.items()}


def _sorted(rec, count):
    from dreg_nerf_amd import ngp_train
    return ngp_train.canonical_order(rec, count)


def _general(dev, seed=3, model=None):
    import test_hip_ngp_train as T
    f, g = T._block(dev, seed=seed)
    with torch.no_grad():
        f.aabb.copy_(torch.tensor(T.AABB if model is None else model, dtype=torch.float32))
    return f.train(), g, T


def _rays_on(dev, T, n, seed):
    r = T._rays(n, seed=seed)
    return r.origins.to(dev).contiguous(), r.viewdirs.to(dev).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------ 1. forward bits
@pytest.mark.parametrize("jitter", ["zero", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 2000])
def test_forward_bits_equal_the_training_forward(dev, n, jitter):
    from dreg_nerf_amd import ngp_train, render
    f, g, T = _general(dev)
    o, d = _rays_on(dev, T, n, seed=20 + n)
    jit = torch.zeros(n, device=dev) if jitter == "zero" else torch.rand(n, generator=torch.Generator().manual_seed(n)).to(dev)
    dt = ngp_train.render_step_size_of(T.AABB)
    bk = [0.25, 0.5, 1.0]
    with torch.no_grad():
        ref = ngp_train.render_image_train(f, g, render.Rays(o, d), T.AABB, dt, torch.tensor(bk), jitter=jit)
    cap = ngp_train.default_sample_capacity(n, T.AABB, dt)
    rgb, opac, dep, ns, count, _, _ = _raw(dev, f, g, o, d, jit, T.AABB, dt, bk, cap)
    assert torch.equal(rgb, ref[0]) and torch.equal(opac, ref[1].reshape(-1)) and torch.equal(dep, ref[2].reshape(-1))
    assert ns == count == ref[3] and (n == 1 or count > 0)
    out = ngp_train.render_image_train(f, g, render.Rays(o, d), T.AABB, dt, torch.tensor(bk), jitter=jit, backward="samples")
    assert torch.equal(out[0].detach(), ref[0]) and torch.equal(out[1].detach(), ref[1]) and torch.equal(out[2].detach(), ref[2]) and out[3] == ref[3]
    assert out[0].requires_grad and out[1].requires_grad and out[2].requires_grad


# ------------------------------------------------------------------------------------------------------------------------------ 2. the list
def _in_order_sum(ray, ordn, val, n_rays):
    """Per ray, the fp32 sum of val in ord order (one addition per survivor, as the kernel accumulates)."""
    acc = np.zeros(n_rays, np.float32)
    for p in range(int(ordn.max()) + 1 if len(ordn) else 0):
        s = ordn == p
        acc[ray[s]] = acc[ray[s]] + val[s]
    return acc


def test_list_of_a_general_block(dev):
    from dreg_nerf_amd import ngp_train
    f, g, T = _general(dev, model=None)
    n = 2000
    o, d = _rays_on(dev, T, n, seed=31)
    jit = torch.rand(n, generator=torch.Generator().manual_seed(32)).to(dev)
    dt = ngp_train.render_step_size_of(T.AABB)
    bk = [0.25, 0.5, 1.0]
    cap = ngp_train.default_sample_capacity(n, T.AABB, dt)
    rgb, opac, dep, ns, count, rec, _ = _raw(dev, f, g, o, d, jit, T.AABB, dt, bk, cap)
    assert 0 < count <= cap
    s = {k: v.cpu().numpy() for k, v in _sorted(rec, count).items()}
    assert len(s["ray"]) == count
    per_ray = np.bincount(s["ray"], minlength=n)
    start = np.concatenate([[0], np.cumsum(per_ray)])[:-1]
    assert np.array_equal(s["ord"], np.arange(count) - start[s["ray"]]) and s["ray"].min() >= 0 and s["ray"].max() < n
    # x = fl(o + fl(t d)), in fp32 on the CPU (separate product and sum: no fused multiply-add)
    oc, dc = o.cpu(), d.cpu()
    r = torch.from_numpy(s["ray"]).long()
    x = oc[r] + torch.from_numpy(s["t"])[:, None] * dc[r]
    assert torch.equal(x, torch.from_numpy(s["x"]))
    # the last record of a ray against the ray's outputs; sum w in order against the opacity
    last = start + per_ray - 1
    hit = per_ray > 0
    O, Cc, D = opac.cpu().numpy(), rgb.cpu().numpy(), dep.cpu().numpy()
    bkf = np.array(bk, np.float32)
    assert np.array_equal(s["P"][last[hit]] + bkf[None] * (np.float32(1) - O[hit])[:, None], Cc[hit])
    assert np.array_equal(s["Pd"][last[hit]], D[hit])
    assert np.array_equal(_in_order_sum(s["ray"], s["ord"], s["w"], n), O)
    assert not O[~hit].any() and not D[~hit].any() and np.array_equal(Cc[~hit], np.tile(bkf, (int((~hit).sum()), 1)))
    # T_next, P and Pd run on within a ray as the kernel accumulates them
    k = np.nonzero(s["ord"] > 0)[0]
    assert np.array_equal(s["Pd"][k], s["Pd"][k - 1] + s["w"][k] * s["t"][k])
    assert np.array_equal(s["P"][k], s["P"][k - 1] + s["w"][k][:, None] * s["c"][k])
    assert np.all(s["T_next"][k] <= s["T_next"][k - 1]) and np.all(s["c"] == s["c"].astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("dens", ("thin", "dense"))
def test_list_of_the_planted_field_is_the_fp64_marchs(dev, dens):
    case = B.planted_set("random")
    a = G._alpha(dev, dens)                                             # (sets the field's aabb to its own case: before _field)
    f = G._field(dev, dens, case.model).train()
    o, d, jit = (torch.from_numpy(v).to(dev) for v in (case.o, case.d, case.jitter))
    rgb, opac, dep, ns, count, rec, _ = _raw(dev, f, G._grid(case, dev), o, d, jit, case.scene, case.dt, B.BKGD, 1 << 16)
    s = {k: v.cpu().numpy() for k, v in _sorted(rec, count).items()}
    want = RS.planted_records(B.planted(dens), case, a, float(np.float32(1) - np.float32(a)))
    ok = case.ref.decidable & want.firm
    keep_g, keep_w = ok[s["ray"]], ok[want.ray]
    assert ok.mean() >= 0.98 and np.array_equal(s["ray"][keep_g], want.ray[keep_w]) and np.array_equal(s["ord"][keep_g], want.ord[keep_w])
    m = case.ref
    f32 = np.float32
    t32 = (case.tmin32().astype(f32)[m.ray] + ((m.n_idx.astype(f32) + f32(0.5)) * f32(case.dt)).astype(f32)).astype(f32)
    assert np.array_equal(s["t"][keep_g], t32[want.kept][keep_w])
    assert (dens == "thin") == bool(want.surv.all())                   # the dense field stops rays early: kept samples that are not listed exist
    assert np.abs(s["w"][keep_g] - want.w[keep_w]).max() <= (int(m.n_model.max()) + 2) * U


# ------------------------------------------------------------------------------------------------------------------------------ 3. capacity
def test_capacity_guards_every_store(dev):
    from dreg_nerf_amd import ngp_train
    f, g, T = _general(dev)
    n = 129
    o, d = _rays_on(dev, T, n, seed=41)
    jit = torch.rand(n, generator=torch.Generator().manual_seed(42)).to(dev)
    dt = ngp_train.render_step_size_of(T.AABB)
    bk = [1.0, 1.0, 1.0]
    full = _raw(dev, f, g, o, d, jit, T.AABB, dt, bk, ngp_train.default_sample_capacity(n, T.AABB, dt))
    count = full[4]
    assert count > 50
    fs =_sorted(full[5], count)
    key_full = set(((fs["ray"].long() << 32) | fs["ord"].long()).tolist())
    rows_full = {int(k): tuple(torch.cat([fs[c][i].reshape(-1) for c in RECORD[2:]]).tolist())
                 for i, k in enumerate(((fs["ray"].long() << 32) | fs["ord"].long()).tolist())}
    for cap in (0, count - 1, count):
        rgb, opac, dep, ns, cnt, rec, band = _raw(dev, f, g, o, d, jit, T.AABB, dt, bk, cap)
        assert torch.equal(rgb, full[0]) and torch.equal(opac, full[1]) and torch.equal(dep, full[2])
        assert ns == cnt == count
        for k in RECORD:
            sent = SENT_I if k in ("ray", "ord") else SENT_F
            assert bool((band[k] == sent).all()), (cap, k)                  # nothing is written behind the capacity
        part = {k: v.cpu() for k, v in rec.items()}
        keys = ((part["ray"].long() << 32) | part["ord"].long()).tolist()
        assert len(set(keys)) == cap and set(keys) <= key_full          # distinct records of the full list, every slot below the capacity written
        for i, k in enumerate(keys):
            assert rows_full[k] == tuple(torch.cat([part[c][i].reshape(-1) for c in RECORD[2:]]).tolist())


def _wrapper_grads(f, g, rays, aabb, dt, bk, jit, coef, **kw):
    from dreg_nerf_amd import ngp_train
    f.mlp_base.params.grad = None
    f.color_mlp.params.grad = None
    rgb, opac, dep, ns = ngp_train.render_image_train(f, g, rays, aabb, dt, bk, jitter=jit, backward="samples", **kw)
    loss = 0.0
    if coef[0] is not None:
        loss = loss + (rgb * coef[0]).sum()
    if coef[1] is not None:
        loss = loss + (opac.squeeze(-1) * coef[1]).sum()
    if coef[2] is not None:
        loss = loss + (dep.squeeze(-1) * coef[2]).sum()
    loss.backward()
    gb = f.mlp_base.params.grad
    gc = f.color_mlp.params.grad
    return gb.clone(), (torch.zeros_like(f.color_mlp.params) if gc is None else gc.clone()), ns


def test_wrapper_relaunches_once_when_the_list_does_not_fit(dev):
    from dreg_nerf_amd import ngp_train, render
    f, g, T = _general(dev, seed=7)
    n = 500
    o, d = _rays_on(dev, T, n, seed=43)
    jit = torch.rand(n, device=dev)
    dt = ngp_train.render_step_size_of(T.AABB)
    coef = (torch.randn(n, 3, device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev))
    b0, c0, n0 = _wrapper_grads(f, g, render.Rays(o, d), T.AABB, dt, torch.ones(3), jit, coef)
    b1, c1, n1 = _wrapper_grads(f, g, render.Rays(o, d), T.AABB, dt, torch.ones(3), jit, coef, sample_capacity=1)
    assert n0 == n1 > 1 and c0.abs().sum() > 0
    assert torch.equal(b0[:3072], b1[:3072]) and torch.equal(c0, c1)
    torch.testing.assert_close(b1[3072:], b0[3072:], rtol=1e-4, atol=1e-5 * float(b0[3072:].abs().max()))


# ------------------------------------------------------------------------------------------------------------------------------ 4. the sample gradients
# fp32 roundings on the longest path from a term to an element, counted from ngp_samples_grad_kernel on the kernel's own records (the inputs
# are exact: the reference is the fp64 rule on the same fp32 values):
#   T * c, rgb - P, the difference, gr * (..)             4      the colour and the depth term alike; the opacity term: 1 - O, * g_O = 2
#   a.dt * dsig                                            1
#   g_c = w * gr                                           1
SG_C_SIGMA, SG_C_COLOUR = 5, 1


def _gpu_records_as_restatement(s, rgb, opac, dep):
    rec = RS.Records()
    for k in ("ray", "ord"):
        setattr(rec, k, s[k].astype(np.int64))
    for k in ("t", "T_next", "w", "c", "P", "Pd"):
        setattr(rec, k, s[k].astype(np.float64))
    rec.T_k = rec.T_next
    rec.C, rec.O, rec.D = rgb.astype(np.float64), opac.astype(np.float64), dep.astype(np.float64)
    rec.bkgd = np.zeros(3)
    return rec


@pytest.mark.parametrize("which", ["rgb", "opacity", "depth", "all"])
def test_samples_grad_within_the_counted_roundings(dev, which):
    from dreg_nerf_amd import ngp_train
    case = B.planted_set("random")
    f = G._field(dev, "dense", case.model).train()
    o, d, jit = (torch.from_numpy(v).to(dev) for v in (case.o, case.d, case.jitter))
    n = len(case.o)
    rgb, opac, dep, ns, count, rec, _ = _raw(dev, f, G._grid(case, dev), o, d, jit, case.scene, case.dt, B.BKGD, 1 << 16)
    srt = _sorted(rec, count)
    rng = np.random.default_rng(5)
    ups = [rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)]
    use = {"rgb": (0,), "opacity": (1,), "depth": (2,), "all": (0, 1, 2)}[which]
    ups = [u if i in use else None for i, u in enumerate(ups)]
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    dirs, gs, gc = ngp_train.samples_grad(srt, d, rgb, opac, dep, t(ups[0]), t(ups[1]), t(ups[2]), case.dt)
    s = {k: v.cpu().numpy() for k, v in srt.items()}
    r64 = _gpu_records_as_restatement(s, rgb.cpu().numpy(), opac.cpu().numpy(), dep.cpu().numpy())
    want_s, want_c, M, terms = RS.sample_grads64(r64, ups[0], ups[1], ups[2], case.dt)
    bound = (SG_C_SIGMA + terms) * U * M
    err = np.abs(gs.cpu().numpy().astype(np.float64) - want_s)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    assert np.all(err[bound == 0] == 0)
    bound_c = (SG_C_COLOUR + 1) * U * np.abs(want_c)
    err_c = np.abs(gc.cpu().numpy().astype(np.float64) - want_c)
    ratio_c = float((err_c[bound_c > 0] / bound_c[bound_c > 0]).max()) if (bound_c > 0).any() else 0.0
    print(f"RATIO samples_grad {which}: dL/dsigma {ratio:.3e}, dL/dc {ratio_c:.3e} over {count} records")
    _note(f"samples_grad {which}", {"g_sigma": ratio, "g_c": ratio_c})
    assert ratio <= 1.0 and ratio_c <= 1.0 and np.all(err_c[bound_c == 0] == 0)
    assert torch.equal(dirs, d[srt["ray"].long()]) and float(np.abs(want_s).sum()) > 0
    if 0 not in use:
        assert not gc.any()


def test_samples_grad_with_all_three_null_writes_nothing(dev):
    from dreg_nerf_amd import lib as L
    n = 100
    ray = torch.zeros(n, dtype=torch.int32, device=dev)
    one, three = torch.ones(n, device=dev), torch.ones(n, 3, device=dev)
    dirs, gs, gc = torch.full((n, 3), SENT_F, device=dev), torch.full((n,), SENT_F, device=dev), torch.full((n, 3), SENT_F, device=dev)
    rc = L.load().dreg_ngp_samples_grad(n, L.ptr(ray), L.ptr(one), L.ptr(one), L.ptr(one), L.ptr(three), L.ptr(three), L.ptr(one), L.ptr(three[:1].contiguous()),
                                        L.ptr(three[:1].contiguous()), L.ptr(one[:1].contiguous()), L.ptr(one[:1].contiguous()), None, None, None, 0.01,
                                        L.ptr(dirs), L.ptr(gs), L.ptr(gc), L.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((dirs == SENT_F).all()) and bool((gs == SENT_F).all()) and bool((gc == SENT_F).all())


# ------------------------------------------------------------------------------------------------------------------------------ 5. the whole backward
# fp32 roundings on the longest path from a term to an element: tests/test_hip_field_train.py's count of ngp_points_bwd_kernel, with the
# roundings in front of its two upstream gradients added (K = the largest number of in-model survivors of a ray of the launch):
#   T_s *= (1 - alpha), w = alpha T_s                      K + 1  (tests/test_hip_render_bwd_fp64.py)
#   t = fl(t_min + fl((n + 1/2) dt))                       4      against the restatement's fp64 t_mid (tests/march_restatement.py: 4u t)
#   forward rgb / depth = sum w c + bkgd (1 - sum w)       3      beyond w and the K additions (counted with T)
#   the term of ngp_samples_grad_kernel                    4 + 5  SG_C_SIGMA less dt's product, and up to five accumulated terms
#   a.dt * dsig                                            1
#   g_c = w * gr                                           K + 2
def counts(K, h0):
    g_sigma = (K + 1) + 4 + 3 + 4 + 5 + 1
    g_c = K + 2
    dO = g_c + 2
    dh0 = g_sigma + 3 + 2 * math.ceil(abs(h0 - 1.0))
    d2 = dO + 4
    d1 = d2 + 64
    dout = d1 + 64
    dh = max(dh0, dout) + 16
    de = dh + 64
    return {"c3": dO + 1, "c2": d2 + 1, "c1": d1 + 1, "d2_row0": dh0 + 1, "d2": dout + 1, "d1": dh + 1, "table": de + 4}


def bounds(res, K, h0):
    """tests/test_hip_field_train.bounds with the counts above: res.M / res.n are the sums of absolute terms and the accumulated terms."""
    c = counts(K, h0)
    b = {k: (c[k] + res.n[k]) * U * res.M[k] for k in ("c3", "c2", "c1", "d1")}
    cd2 = np.full((16, 1), float(c["d2"]))
    cd2[0] = c["d2_row0"]
    b["d2"] = (cd2 + res.n["d2"]) * U * res.M["d2"]
    b["c1"][:, :16] += 2.0 ** -11 * res.M["c1"][:, :16]               # the kernel's fp16 SH value may differ from the oracle's by an ulp
    b["table"] = (c["table"] + res.t_n) * U * res.t_M
    return b


RATIO_WORST = {}


def _note(label, ratios):
    """The largest observed ratio per launch and over the run, beside the committed summary (profiles/render_samples_fp64_ratios.txt), to a path
    git ignores: the table entries' last bits depend on the order of the atomics."""
    RATIO_WORST[label] = max(ratios.items(), key=lambda kv: kv[1])
    worst = max(RATIO_WORST.values(), key=lambda kv: kv[1])
    try:
        with open(os.path.join(ROOT, "profiles", "render_samples_fp64_ratios.latest.txt"), "w") as fh:
            fh.write("largest |gpu - fp64| / ((C + n) 2^-24 M), tests/test_hip_render_samples.py\n")
            fh.write("".join(f"{lb}: {v:.3e} ({k})\n" for lb, (k, v) in RATIO_WORST.items()) + f"largest observed: {worst[1]:.3e} ({worst[0]})\n")
    except OSError:
        pass


def _upstream(case, which, every=1, seed=17):
    """Upstream gradients of the rays (None where the term is absent); rays whose kept set a rounding could change, and with every > 1 all but
    every `every`-th ray and the rays at the lane and chunk edges, carry 0."""
    n = len(case.o)
    rng = np.random.default_rng(seed)
    g = [B.g_rgb_of(case), rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)]
    on = case.ref.decidable.copy()
    if every > 1:
        pick = np.zeros(n, bool)
        pick[::every] = True
        pick[[p for p in B.EDGE_LANES + (n - 1,) if p < n]] = True
        on &= pick
    use = {"rgb": (0,), "opacity": (1,), "depth": (2,), "all": (0, 1, 2)}[which]
    return [(g[i] * (on[:, None] if i == 0 else on)).astype(np.float32) if i in use else None for i in range(3)], on


def _compare(dev, dens, case, label, which="all", every=1):
    from dreg_nerf_amd import render as R
    a = G._alpha(dev, dens)
    q = float(np.float32(1) - np.float32(a))
    r = case.ref
    p = B.planted(dens)
    ups, on = _upstream(case, which, every)
    f = G._field(dev, dens, case.model).train()
    levels = GR.levels_from_ctypes(f._levels)
    rec = RS.planted_records(p, case, a, q)
    assert rec.firm[r.n_kept > 0].all()
    full = B.record_of(p, case, r)
    record = {k: (v[rec.kept] if k in ("xin", "x") else v) for k, v in full.items()}
    live = on[rec.ray]                                                  # the rest adds exactly nothing: left out of the reference
    sub = RS.Records()
    for k in ("ray", "ord", "kept", "t", "T_k", "T_next", "w", "c", "P", "Pd"):
        setattr(sub, k, getattr(rec, k)[live])
    sub.C, sub.O, sub.D, sub.bkgd = rec.C, rec.O, rec.D, rec.bkgd
    record = {k: (v[live] if k in ("xin", "x") else v) for k, v in record.items()}
    val, ab = RS.whole_backward64(sub, record, p["weights"], ups[0], ups[1], ups[2], case.dt, levels, case.model)
    if which == "rgb":                                                  # with g_rgb alone the reference is the ray backward's own restatement
        old = RB.backward64(full, p["weights"], r, a, q, ups[0], B.BKGD, case.dt, levels, case.model)
        for k in RB.MATRICES:
            assert np.abs(old.val[k] - val.val[k]).max() <= 1e-9 * max(1.0, np.abs(old.val[k]).max()), k
        assert np.array_equal(old.t_idx, val.t_idx) and np.abs(old.t_val - val.t_val).max() <= 1e-9 * max(1.0, np.abs(old.t_val).max())
        val = old
    t = lambda x: None if x is None else torch.from_numpy(x).to(dev)
    rays = R.Rays(torch.from_numpy(case.o).to(dev), torch.from_numpy(case.d).to(dev))
    gb, gc, ns = _wrapper_grads(f, G._grid(case, dev), rays, case.scene, case.dt, torch.tensor(B.BKGD), torch.from_numpy(case.jitter).to(dev),
                                [t(u) for u in ups])
    gb, gc = gb.cpu().numpy(), gc.cpu().numpy()
    if r.decidable.all():
        assert ns == int(rec.surv.sum())
    K = int(r.n_model.max())
    bnd = bounds(ab, K, B.H0[dens])
    got = {"d1": gb[:2048].reshape(64, 32), "d2": gb[2048:3072].reshape(16, 64), "c1": gc[:2048].reshape(64, 32),
           "c2": gc[2048:6144].reshape(64, 64), "c3": gc[6144:6144 + 192].reshape(3, 64)}
    assert not gc[6144 + 192:].any()                                    # rows 3..15 of colour W3
    assert np.array_equal(val.t_idx, ab.t_idx)
    tab = gb[3072:].copy()
    got_t = tab[val.t_idx].astype(np.float64)
    tab[val.t_idx] = 0.0
    stray = np.nonzero(tab)[0]
    assert len(stray) == 0, (len(stray), stray[:16].tolist())           # untouched entries are exactly 0
    blocks = [(k, got[k].astype(np.float64), val.val[k], bnd[k]) for k in RB.MATRICES]
    blocks.insert(3, ("c1 sh", blocks[2][1][:, :16], blocks[2][2][:, :16], blocks[2][3][:, :16]))
    blocks[2] = ("c1 feat+1", blocks[2][1][:, 16:], blocks[2][2][:, 16:], blocks[2][3][:, 16:])
    for l in range(16):
        s = val.t_level == l
        blocks.append((f"table {l}", got_t[s], val.t_val[s], bnd["table"][s]))
    ratios = {}
    for name, x, want, b in blocks:
        err = np.abs(x - want)
        assert np.all(x[b == 0] == 0), name                             # no term: exactly 0
        ratios[name] = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"RATIO {label} {dens} {which} (K {K}, {int(rec.surv.sum())} survivors, {int(live.sum())} with gradient, {len(val.t_idx)} table elements): "
          + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    _note(f"{label} {dens} {which}", ratios)
    bad = {k: v for k, v in ratios.items() if v > 1.0}
    assert not bad, bad
    assert len(val.t_idx) > 0 and np.abs(got["d1"]).sum() > 0 and np.abs(got["d2"]).sum() > 0
    if which in ("rgb", "all"):
        assert all(np.abs(got[k]).sum() > 0 for k in RB.MATRICES)
    else:
        assert not gc.any()                                             # opacity and depth do not depend on the colour net
    return ns


@pytest.mark.parametrize("dens", ("thin", "dense"))
@pytest.mark.parametrize("n", B.EDGE_COUNTS)
def test_whole_backward_at_lane_and_chunk_edges(dev, n, dens):
    _compare(dev, dens, B.edge_set(n), f"{n} rays", "all")


@pytest.mark.parametrize("which", ["rgb", "opacity", "depth"])
def test_whole_backward_term_by_term(dev, which):
    _compare(dev, "dense", B.edge_set(129), "129 rays", which)


@functools.lru_cache(maxsize=None)
def long_list_set():
    """The four 4,500-ray training sets of the ragged grid (one per jitter of march_cases.JITTERS): 18,000 rays whose thin-density list, where
    no ray stops early, holds more than 131,072 samples, the length at which a chunk of dreg_ngp_points_bwd holds 128 points."""
    parts = [C.random_case("ragged", B.DT, j) for j in C.JITTERS]
    cat = lambda k: np.concatenate([getattr(c, k) for c in parts])
    c0 = parts[0]
    return C.Case("samples-long-list", c0.binary, c0.roi, c0.scene, c0.model, cat("o"), cat("d"), c0.dt, jitter=cat("jitter"))


def test_whole_backward_beyond_131072_samples(dev):
    case = long_list_set()
    ns = _compare(dev, "thin", case, f"{len(case.o)} rays", "all", every=8)
    assert ns > 131072


def test_all_miss_launch_is_exactly_zero(dev):
    from dreg_nerf_amd import render as R
    case = B.miss_set()
    f = G._field(dev, "thin", case.model).train()
    n = len(case.o)
    rays = R.Rays(torch.from_numpy(case.o).to(dev), torch.from_numpy(case.d).to(dev))
    coef = (torch.randn(n, 3, device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev))
    gb, gc, ns = _wrapper_grads(f, G._grid(case, dev), rays, case.scene, case.dt, torch.tensor(B.BKGD), torch.from_numpy(case.jitter).to(dev), coef)
    assert ns == 0 and not gb.any() and not gc.any()


# ------------------------------------------------------------------------------------------------------------------------------ 6. general field
@pytest.mark.parametrize("model_inside", [False, True], ids=["model_is_scene", "model_inside_scene"])
def test_general_field_matches_cpu_autograd_with_the_three_term_loss(dev, model_inside):
    """tests/test_hip_ngp_train.py::test_backward_matches_cpu_autograd with L = sum a . rgb + b opacity + c depth: the same block, rays and
    thresholds (cosine >= 0.999, relative L2 <= 2e-2 per matrix, per column group of colour W1 and per table level), on the rays whose forward
    agrees with the CPU restatement's (>= 99 %)."""
    from dreg_nerf_amd import ngp_train, render
    import test_hip_ngp_train as T
    model = T.MODEL_INSIDE if model_inside else T.AABB
    f, g, _ = _general(dev, seed=3, model=model)
    n, dt, bk = 300, 0.02, torch.ones(3)
    rays = T._rays(n, seed=4)
    jitter = torch.rand(n, generator=torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(6)
    coef = [torch.randn(n, 3, generator=gen) / n, torch.randn(n, generator=gen) / n, torch.randn(n, generator=gen) / n]
    rays_d = render.Rays(rays.origins.to(dev), rays.viewdirs.to(dev))

    def cpu(mask):
        base = f.mlp_base.params.detach().cpu().clone().requires_grad_(True)
        color = f.color_mlp.params.detach().cpu().clone().requires_grad_(True)
        rgb, opac, depth, surv = RT.render_train(base, color, model, rays.origins, rays.viewdirs, g.binary.cpu(), T.AABB, T.AABB, dt, jitter, bk)
        ((rgb * coef[0] * mask[:, None]).sum() + (opac * coef[1] * mask).sum() + (depth * coef[2] * mask).sum()).backward()
        return rgb.detach(), opac.detach(), depth.detach(), base.grad, color.grad, surv

    rgb_c, opac_c, dep_c, _, _, surv_c = cpu(torch.zeros(n))
    f.mlp_base.params.grad = None
    f.color_mlp.params.grad = None
    rgb, opac, dep, ns = ngp_train.render_image_train(f, g, rays_d, T.AABB, dt, bk, jitter=jitter.to(dev), backward="samples")
    cap = ngp_train.default_sample_capacity(n, T.AABB, dt)
    rec = _raw(dev, f, g, rays_d.origins.contiguous(), rays_d.viewdirs.contiguous(), jitter.to(dev), T.AABB, dt, [1.0, 1.0, 1.0], cap)
    per_ray = torch.bincount(rec[5]["ray"][:rec[4]].long().cpu(), minlength=n)
    assert int(per_ray.sum()) == ns
    agree = (per_ray == surv_c.sum(1)) & ((rgb.detach().cpu() - rgb_c).abs().max(-1).values < 2e-3)
    assert agree.float().mean() >= 0.99, f"forward agrees on {agree.float().mean():.3f} of the rays"
    mask = agree.float()
    md = mask.to(dev)
    ((rgb * coef[0].to(dev) * md[:, None]).sum() + (opac.squeeze(-1) * coef[1].to(dev) * md).sum() + (dep.squeeze(-1) * coef[2].to(dev) * md).sum()).backward()
    gb, gc = f.mlp_base.params.grad.cpu(), f.color_mlp.params.grad.cpu()
    _, _, _, rb, rc, _ = cpu(mask)
    touched = RT.reached_entries(agree)
    failed = []
    for what, (which, idx) in T.blocks_of(gb, gc, touched).items():
        cos, r = T.cos_rel((gb, gc)[which][idx], (rb, rc)[which][idx])
        print(f"BLOCK {what}: cosine {cos:.6f}, rel L2 {r:.3e}")
        if not (cos >= 0.999 and r <= 2e-2):
            failed.append(f"{what}: cosine {cos:.5f}, rel L2 {r:.3e}")
    assert not failed, failed
    assert torch.count_nonzero(gc[6144 + 192:]) == 0


def test_mlp_gradients_deterministic_across_runs_and_forward_widths(dev):
    from dreg_nerf_amd import lib as L, ngp_train, render
    f, g, T = _general(dev, seed=7)
    n = 5000
    o, d = _rays_on(dev, T, n, seed=8)
    jit = torch.rand(n, device=dev)
    dt = ngp_train.render_step_size_of(T.AABB)
    coef = (torch.randn(n, 3, device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev))
    run = lambda: _wrapper_grads(f, g, render.Rays(o, d), T.AABB, dt, torch.ones(3), jit, coef)
    b0, c0, n0 = run()
    b1, c1, n1 = run()
    assert n0 == n1 and torch.equal(b0[:3072], b1[:3072]) and torch.equal(c0, c1)
    with L.probe() as p:
        for w in (1, 7, 300):
            p.set("dreg_render_samples_set_waves", w, 2048)
            bw, cw, nw = run()
            assert nw == n0 and torch.equal(b0[:3072], bw[:3072]) and torch.equal(c0, cw), f"width {w}"
            torch.testing.assert_close(bw[3072:], b0[3072:], rtol=1e-4, atol=1e-5 * float(b0[3072:].abs().max()))
    assert c0.abs().sum() > 0 and b0[3072:].abs().sum() > 0


@pytest.mark.parametrize("which", ["opacity", "depth"])
def test_opacity_and_depth_losses_reach_the_parameters(dev, which):
    """A loss on the opacity or on the depth alone has a gradient in "samples" mode.  Both depend on the densities only: the gradient reaches
    mlp_base.params (the density net and the hash table); color_mlp.params, which neither output depends on, gets exactly zero."""
    from dreg_nerf_amd import ngp_train, render
    f, g, T = _general(dev, seed=9)
    n = 400
    o, d = _rays_on(dev, T, n, seed=10)
    dt = ngp_train.render_step_size_of(T.AABB)
    f.mlp_base.params.grad = None
    f.color_mlp.params.grad = None
    rgb, opac, dep, ns = ngp_train.render_image_train(f, g, render.Rays(o, d), T.AABB, dt, torch.ones(3), jitter=torch.rand(n, device=dev), backward="samples")
    out = opac if which == "opacity" else dep
    assert out.requires_grad and ns > 0
    ((out.squeeze(-1) - 0.5) ** 2).mean().backward()
    gb, gc = f.mlp_base.params.grad, f.color_mlp.params.grad
    assert gb is not None and bool(torch.isfinite(gb).all())
    assert float(gb[:2048].abs().sum()) > 0 and float(gb[2048:3072].abs().sum()) > 0 and float(gb[3072:].abs().sum()) > 0
    assert gc is not None and not bool(gc.any())


# ------------------------------------------------------------------------------------------------------------------------------ end to end
# Not tuned.  0.5 puts the mask term on the colour term's own scale: smooth-L1 (beta = 1) is 0.5 d^2 per element for |d| < 1, the mask term
# W d^2.  (One run at 0.1: 35.83 dB, free-space opacity 1.69e-3 against 1.98e-3 without; DESIGN.md §3o has the figures of both weights.)
OPACITY_LOSS_WEIGHT = 0.5


def _train_and_measure(root, name, weight):
    """train_ngp_nerf.py --backward samples on the sphere scene: (held-out PSNR, mean rendered opacity over held-out pixels of alpha 0)."""
    import test_hip_ngp_train as T
    from dreg_nerf_amd import render
    from dreg_nerf_amd.nerf_images import SubjectImages
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "train_ngp_nerf.py"), "--dataset", "objaverse", "--root_dir", root, "--scene", "sphere", "--expname", name,
           "--max_iterations", str(T.ITERS), "--n_validation", str(T.ITERS), "--n_checkpoint", str(T.ITERS), "--backward", "samples",
           "--opacity_loss_weight", str(weight)]
    out = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    m = re.findall(r"val psnr ([0-9.]+)", out.stdout)
    assert m, out.stdout[-2000:]
    dev = torch.device("cuda:0")
    field, grid, meta = render.load_render_block(os.path.join(root, "out", name, "model.pth"), dev)
    val = SubjectImages.load("objaverse", root, "sphere", "test", dev)[0]
    field.eval()
    tot, cnt = 0.0, 0
    with torch.no_grad():
        for i in range(len(val)):
            rays, _ = val.view(i)
            _, acc, _, _ = render.render_image(field, grid, rays, meta["aabb_host"], render_step_size=float(meta["render_step_size"]),
                                               render_bkgd=torch.ones(3))
            empty = val.images[i, :, :, 3] == 0
            tot += float(acc[..., 0][empty].sum())
            cnt += int(empty.sum())
    assert cnt > 1000
    return float(m[-1]), tot / cnt


def test_train_ngp_nerf_with_the_sample_list_and_the_mask_loss(tmp_path):
    """tests/test_hip_ngp_train.py's sphere scene through train_ngp_nerf.py --backward samples, 600 steps, once with --opacity_loss_weight 0 and once
    with OPACITY_LOSS_WEIGHT: both meet that test's floor (30.0 dB; the ray backward's own figure on this scene is 35.39 dB), and the mean
    rendered opacity over the held-out pixels whose ground-truth alpha is 0 is not above the run's without the mask loss."""
    import test_hip_ngp_train as T
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    root = str(tmp_path)
    T._write_scene(root, "sphere")
    psnr0, free0 = _train_and_measure(root, "w0", 0.0)
    psnr1, free1 = _train_and_measure(root, "w1", OPACITY_LOSS_WEIGHT)
    print(f"E2E samples: W = 0: {psnr0:.2f} dB, free-space opacity {free0:.3e}; W = {OPACITY_LOSS_WEIGHT}: {psnr1:.2f} dB, free-space opacity {free1:.3e}")
    try:
        with open(os.path.join(ROOT, "profiles", "render_samples_e2e.latest.txt"), "w") as fh:
            fh.write(json.dumps({"iters": T.ITERS, "W": OPACITY_LOSS_WEIGHT, "psnr_w0": psnr0, "free_opacity_w0": free0, "psnr_w": psnr1, "free_opacity_w": free1}) + "\n")
    except OSError:
        pass
    assert psnr0 >= T.PSNR_FLOOR and psnr1 >= T.PSNR_FLOOR, (psnr0, psnr1)
    assert free1 <= free0, (free1, free0)
