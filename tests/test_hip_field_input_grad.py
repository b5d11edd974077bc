"""GPU: the field's input gradients of csrc/field_input_grad.hip (dreg_ngp_points_input_grad, dreg_ngp_samples_ray_grad) and what
is built on them.

1. Planted field, element by element against the fp64 restatement of tests/field_input_grad_restatement.py at 1, 63, 64, 65 and 129 points with
   gradient only at points 0, 62, 63, 64, 127, 128 and the last, the hits in turn inside the model aabb, outside on one axis and outside on
   three: every element of dL/dx and dL/ddir within (C + n) 2^-24 M, M the sum of the absolute terms, n the terms of the element's last sum, C
   the fp32 roundings on the longest path from a term to the element, counted from the kernel's source in counts() below.  The field's table is
   NOT constant across a cell's corners (a constant table makes dL/dx exactly 0 and the test blind): all parameters are uniform random, so the
   forward is a general one.  The reference takes from the DEVICE's forward what the rule takes from the forward as values, h0 and the fp16
   colour c (the kernel's own record, as tests/test_hip_render_samples.py does), and the three ReLU gates from the oracle's forward on the device's
   raw features; the hits are chosen so that every pre-activation is at least GATE_MARGIN from 0, far beyond what the fp32 sums or an ulp of an
   fp16 SH value can move it, and the test asserts that margin on the device's values first.
   tests/test_field_input_grad_host.py shows that seven deliberate errors each land well beyond this bound.
2. Exact zeros.   3. A general field against CPU autograd through oracle.ngp_oracle.   4. The ray level: dreg_ngp_samples_ray_grad against the
restatement, determinism across runs and forward launch widths, and the existing outputs and parameter gradients bit for bit with and without
requires_grad on the inputs.   5. Pose recovery against autograd as the yardstick.   6. The product through eval_nerf_regtr.py's main()."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_input_grad_restatement as IG
import field_points_restatement as FP
import render_bwd_cases as B
from oracle import ngp_oracle as N

gpu = pytest.mark.gpu
U = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------------ the planted cases (CPU and GPU)
MODEL = [-1.0, -0.75, -1.25, 1.0, 1.25, 0.75]            # the model aabb, strictly inside the sampled box
BOX = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
EDGE_COUNTS = (1, 63, 64, 65, 129)
HIT_LANES = (0, 62, 63, 64, 127, 128)                    # with point n - 1: the only points that carry upstream gradient
GATE_MARGIN = 2.0 ** -9                                  # every pre-activation of a hit is at least this far from 0 (chosen so; asserted)


@functools.lru_cache(maxsize=None)
def plant_params():
    """The planted field's parameters: everything uniform random (table in (-0.5, 0.5): not constant across any cell's corners)."""
    gen = torch.Generator().manual_seed(5)
    base = torch.empty(3072 + N.n_grid_params()).uniform_(-0.5, 0.5, generator=gen)
    base[:3072].uniform_(-0.3, 0.3, generator=gen)
    color = torch.empty(7168).uniform_(-0.3, 0.3, generator=gen)
    return base, color


@functools.lru_cache(maxsize=None)
def plant_table():
    return N.f16(plant_params()[0][3072:]).numpy().reshape(-1, 2)


def plant_record(x, d, raw=None, c=None):
    """(record, weights, margin [N]): the oracle's forward record of the planted field at the points, with the colour net re-evaluated (fp64 sums
    between fp16 roundings) on `raw` when given (the device's own fp16 h0 | 15 features) and c replaced by the device's; margin = the smallest
    |pre-activation| of the point over the three hidden layers."""
    base, color = plant_params()
    rec, W, _ = FP.forward_record(x, d, base, color, MODEL)
    f16 = lambda a: a.astype(np.float16).astype(np.float64)
    if raw is not None:
        rec["raw"] = np.asarray(raw, np.float64)
    xin = rec["xin"].copy()
    xin[:, 16:31] = rec["raw"][:, 1:16]
    pre_hd = rec["enc"] @ W["d1"].T
    pre_h1 = xin @ W["c1"].T
    h1 = f16(np.maximum(pre_h1, 0.0))
    pre_h2 = h1 @ W["c2"].T
    rec.update(xin=xin, hd=np.maximum(pre_hd, 0.0), h1=h1, h2=f16(np.maximum(pre_h2, 0.0)))
    if c is not None:
        rec["c"] = np.asarray(c, np.float64)
    margin = np.minimum(np.minimum(np.abs(pre_hd).min(1), np.abs(pre_h1).min(1)), np.abs(pre_h2).min(1))
    return rec, W, margin


class PlantCase:
    pass


@functools.lru_cache(maxsize=None)
def plant_case(n, seed=31):
    """n points uniform in BOX with unit Gaussian directions; upstream gradients (both) only at HIT_LANES and n - 1; the hits in turn inside
    MODEL, outside on one axis, outside on three (the first one inside), each the first of 256 candidates of its kind whose gates keep
    2 GATE_MARGIN on the oracle's forward (the GPU test asserts GATE_MARGIN on the device's)."""
    rng = np.random.default_rng(seed + n)
    lo, hi = np.array(BOX[:3]), np.array(BOX[3:])
    mlo, mhi = np.array(MODEL[:3]), np.array(MODEL[3:])
    c = PlantCase()
    c.n = n
    c.x = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.standard_normal((n, 3))
    c.d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    c.hits = np.array(sorted({p for p in HIT_LANES + (n - 1,) if p < n}))
    c.kind = np.array([rank % 3 for rank in range(len(c.hits))])
    for rank, h in enumerate(c.hits):
        cand = mlo + (0.1 + 0.8 * rng.random((256, 3))) * (mhi - mlo)
        if c.kind[rank] == 1:
            k = rank % 3
            cand[:, k] = mhi[k] + 0.05 + 0.15 * rng.random(256)
        elif c.kind[rank] == 2:
            cand = mhi + 0.05 + 0.15 * rng.random((256, 3))
            cand[:, rank % 3] = mlo[rank % 3] - 0.05 - 0.15 * rng.random(256)
        cd = rng.standard_normal((256, 3))
        cd = (cd / np.linalg.norm(cd, axis=1, keepdims=True)).astype(np.float32)
        _, _, margin = plant_record(cand.astype(np.float32), cd)
        ok = np.nonzero(margin >= 2 * GATE_MARGIN)[0]
        assert len(ok), (n, rank)
        c.x[h], c.d[h] = cand[ok[0]].astype(np.float32), cd[ok[0]]
    c.g_sigma = np.zeros(n, np.float32)
    c.g_rgb = np.zeros((n, 3), np.float32)
    c.g_sigma[c.hits] = rng.standard_normal(len(c.hits)).astype(np.float32)
    c.g_rgb[c.hits] = rng.standard_normal((len(c.hits), 3)).astype(np.float32)
    return c


def plant_reference(case, use_sigma=True, use_rgb=True, mutate=None, raw=None, col=None):
    """input_grad64 over the points that carry gradient (every other row is exactly zero): (result, record, margin)."""
    rows = case.hits
    rec, W, margin = plant_record(case.x[rows], case.d[rows], raw, col)
    res = IG.input_grad64(rec, W, plant_table(), case.d[rows], case.g_sigma[rows] if use_sigma else None, case.g_rgb[rows] if use_rgb else None,
                          B.levels(), MODEL, mutate=mutate)
    return res, rec, margin


# fp32 roundings on the longest path from a term to an element, counted from ngp_points_input_grad_kernel (csrc/field_input_grad.hip).  The
# chain up to de is ngp_points_bwd_kernel's (tests/test_hip_field_train.py: the MFMA v_mfma_f32_16x16x4_f32 is a chain of fused multiply-adds,
# one rounding per step, K steps for a K-term product-sum; 1 - c and h0 - 1 are exact; -ffp-contract=off):
#   dO = gc * c * (1 - c)                                  2
#   dh0 = gs * __expf(x), x = h0 - 1                       1 + 2 + 2 ceil|x|
#   d2 = dO W3[0:4] (K = 4)   4        d1 = d2 W2 (K = 64)   64        dsh, dout[1..15] = d1 W1 (K = 64)   64
#   dh = dout W2d (K = 16)   16        de = dh W1d (K = 64)   64
# the direction tail: a monomial of dsh4/dd times dsh[j] is at most 6 roundings (2 for the squares or products of two coordinates, up to 3
#   for the constant's products, 1 for the product with dsh[j]); its sums are the n of the element                                        6
# the position tail: v = f0 t0 + f1 t1 (3), 1 - w (1), w_a w_b (1), times v (1), scale_l D (1), hi - lo (1), the quotient (1)             9
#   and 16 levels x 8 corners x 2 features = 256 terms of the element's sums
def counts(h0):
    h0 = np.asarray(h0, np.float64)
    dO = 2.0
    dh0 = 3.0 + 2.0 * np.ceil(np.abs(h0 - 1.0))
    d1 = dO + 4 + 64
    dsh = dout = d1 + 64
    dh = np.maximum(dh0, dout) + 16
    de = dh + 64
    return {"dir": dsh + 6, "x": de + 9}


def bounds(res, h0):
    c = counts(h0)
    return (c["x"][:, None] + res.nx) * U * res.gxM, (c["dir"] + res.nd) * U * res.gdM


# ------------------------------------------------------------------------------------------------------------------------------ the GPU side
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


_PLANT = {}


def _plant_field(dev):
    from dreg_nerf_amd import ngp
    if "f" not in _PLANT:
        base, color = plant_params()
        f = ngp.NGPradianceField(MODEL)
        with torch.no_grad():
            f.mlp_base.params.copy_(base)
            f.color_mlp.params.copy_(color)
        _PLANT["f"] = f.to(dev)
    return _PLANT["f"]


def _launch(dev, f, x, d, gs, gc, want_x=True, want_dir=True):
    """The C entry itself on outputs pre-filled with NaN: what comes back was WRITTEN by the call."""
    from dreg_nerf_amd import lib as L
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt, dt_, gst, gct = t(x), t(d), t(gs), t(gc)
    n = len(x)
    gx = torch.full((n, 3), float("nan"), device=dev) if want_x else None
    gd = torch.full((n, 3), float("nan"), device=dev) if want_dir else None
    base16, col16 = f._prepared()
    rc = L.load().dreg_ngp_points_input_grad(L.ptr(xt), L.ptr(dt_), n, base16.data_ptr(), col16.data_ptr(), *f._levels, L.f6(MODEL), L.ptr(gst), L.ptr(gct),
                                             L.ptr(gx), L.ptr(gd), L.stream())
    assert rc == 0
    torch.cuda.synchronize()
    return (None if gx is None else gx.cpu().numpy()), (None if gd is None else gd.cpu().numpy())


def _device_record(dev, f, case):
    """The device's own forward at the hits: raw (fp16 h0 | 15 features) and the fp16 colour."""
    from dreg_nerf_amd import field_train as FT
    x, d = torch.from_numpy(case.x[case.hits]).to(dev), torch.from_numpy(case.d[case.hits]).to(dev)
    with torch.no_grad():
        _, raw = f.query_raw(x)
        _, rgb = FT.field_points(f, x, d)
    return raw.float().cpu().numpy().astype(np.float64), rgb.float().cpu().numpy().astype(np.float64)


RATIO_WORST = {}


def _note(label, ratios):
    RATIO_WORST[label] = ratios
    try:
        with open(os.path.join(ROOT, "profiles", "field_input_grad_fp64_ratios.latest.txt"), "w") as fh:
            fh.write("largest |gpu - fp64| / ((C + n) 2^-24 M), tests/test_hip_field_input_grad.py\n")
            fh.write("".join(f"{lb}: " + ", ".join(f"{k} {v:.3e}" for k, v in r.items()) + "\n" for lb, r in RATIO_WORST.items()))
            fh.write(f"largest observed: {max(v for r in RATIO_WORST.values() for v in r.values()):.3e}\n")
    except OSError:
        pass


@gpu
@pytest.mark.parametrize("n,which", [(n, "both") for n in EDGE_COUNTS] + [(129, "sigma"), (129, "rgb")])
def test_planted_field_within_the_counted_roundings(dev, n, which):
    f = _plant_field(dev)
    case = plant_case(n)
    use_sigma, use_rgb = which != "rgb", which != "sigma"
    raw, col = _device_record(dev, f, case)
    res, rec, margin = plant_reference(case, use_sigma, use_rgb, raw=raw, col=col)
    assert margin.min() >= GATE_MARGIN, margin                              # the gates of the reference are the device's
    inside_hits = case.kind == 0
    assert np.array_equal(res.inside, inside_hits)
    if which == "both":
        assert np.all(np.abs(res.gx[inside_hits]) > 0)                      # the test is not blind: dL/dx is non-zero at every inside hit
    gx, gd = _launch(dev, f, case.x, case.d, case.g_sigma if use_sigma else None, case.g_rgb if use_rgb else None)
    rest = np.setdiff1d(np.arange(n), case.hits)
    assert not gx[rest].any() and not gd[rest].any()                        # rows without upstream gradient: written, exactly 0
    bx, bd = bounds(res, rec["raw"][:, 0])
    gxh, gdh = gx[case.hits].astype(np.float64), gd[case.hits].astype(np.float64)
    assert np.all(gxh[bx == 0] == 0) and np.all(gdh[bd == 0] == 0)          # no term: exactly 0 (a clamped axis, dL/ddir under dL/dsigma alone)
    assert np.all(gxh[~res.open] == 0)
    ratios = {"dL/dx": float((np.abs(gxh - res.gx)[bx > 0] / bx[bx > 0]).max()) if (bx > 0).any() else 0.0,
              "dL/ddir": float((np.abs(gdh - res.gd)[bd > 0] / bd[bd > 0]).max()) if (bd > 0).any() else 0.0}
    print(f"RATIO {n} points, {which} ({len(case.hits)} hits, {int(inside_hits.sum())} inside): " + ", ".join(f"{k} {v:.3e}" for k, v in ratios.items()))
    _note(f"{n} points, {which}", ratios)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if which == "sigma":
        assert not gd.any()                                                 # the density does not see the direction
    if which != "sigma":
        assert np.all(np.abs(gdh) > 0)
        out1 = case.kind == 1                                               # outside on one axis: that axis exactly 0, the other two carry the colour term
        assert np.all((gxh[out1] != 0).sum(1) == 2) and np.all((gxh[case.kind == 2] == 0))


@gpu
def test_exact_zeros(dev):
    """Both upstream pointers null: zeros are written.  A pass none of whose 64 points carries gradient is skipped, its rows written as zeros.
    Either output may be absent.  All-zero upstream arrays give zeros."""
    f = _plant_field(dev)
    case = plant_case(129)
    gx, gd = _launch(dev, f, case.x, case.d, None, None)
    assert not gx.any() and not gd.any()                                    # (NaN-prefilled: these zeros were written)
    gs = np.zeros(129, np.float32)
    gs[128] = 1.0                                                           # passes 0 and 1 are skipped
    gx, gd = _launch(dev, f, case.x, case.d, gs, None)
    assert not gx[:128].any() and not gd.any() and np.isfinite(gx).all()
    assert (gx[128] != 0).any() == bool(case.kind[list(case.hits).index(128)] == 0)      # dL/dsigma alone reaches x only inside the aabb
    gx, gd = _launch(dev, f, case.x, case.d, np.zeros(129, np.float32), np.zeros((129, 3), np.float32))
    assert not gx.any() and not gd.any()
    full_x, full_d = _launch(dev, f, case.x, case.d, case.g_sigma, case.g_rgb)
    only_x, none_d = _launch(dev, f, case.x, case.d, case.g_sigma, case.g_rgb, want_dir=False)
    none_x, only_d = _launch(dev, f, case.x, case.d, case.g_sigma, case.g_rgb, want_x=False)
    assert none_d is None and none_x is None and np.array_equal(only_x, full_x) and np.array_equal(only_d, full_d)
    again_x, again_d = _launch(dev, f, case.x, case.d, case.g_sigma, case.g_rgb)
    assert np.array_equal(again_x, full_x) and np.array_equal(again_d, full_d)           # no atomics: bit-identical between runs


# ------------------------------------------------------------------------------------------------------------------------ the general field
@gpu
@pytest.mark.parametrize("which", ["sigma", "rgb", "both"])
def test_general_field_matches_cpu_autograd(dev, which):
    """4,096 points on the generated 32^3 block (model aabb inside the sampled cube: points outside exist), the whole [N,3] arrays of dL/dx and
    dL/ddir through field_points' autograd: cosine >= 0.999 and relative L2 <= 2e-2 against torch autograd through
    oracle.ngp_oracle.query_density / query_rgb on the CPU (the thresholds of tests/test_hip_field_train.py for this chain), over ALL points."""
    import render_train_restatement as RT
    import test_hip_field_train as G
    from dreg_nerf_amd import field_train as FT
    f, T = G._general(dev)
    n = 4096
    x, d = G._points(n, seed=21)
    f.train()
    xg, dg = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    sigma, rgb = FT.field_points(f, xg, dg)
    gen = torch.Generator().manual_seed(22)
    gs = torch.randn(n, generator=gen) / n * (which != "rgb")
    gc = torch.randn(n, 3, generator=gen) / n * (which != "sigma")
    loss = 0
    if which != "rgb":
        loss = loss + (sigma * gs.to(dev)).sum()
    if which != "sigma":
        loss = loss + (rgb * gc.to(dev)).sum()
    f.mlp_base.params.grad = None
    f.color_mlp.params.grad = None
    loss.backward()
    base, color = f.mlp_base.params.detach().cpu(), f.color_mlp.params.detach().cpu()
    aabb = torch.tensor(T.MODEL_INSIDE, dtype=torch.float32)
    xc, dc = x.clone().requires_grad_(True), d.clone().requires_grad_(True)
    with RT.fp32_backward():
        sig_c, raw_c = N.query_density(xc, aabb, base)
        rgb_c = N.query_rgb(dc, raw_c, color)
        ((sig_c * gs).sum() + (rgb_c * gc).sum()).backward()
    assert int((sig_c.detach() == 0).sum()) > 100                           # points outside the model aabb
    failed = []
    for what, a, b in (("dL/dx", xg.grad.cpu(), xc.grad), ("dL/ddir", dg.grad.cpu(), dc.grad)):
        if which == "sigma" and what == "dL/ddir":
            assert not a.any() and not b.any()
            continue
        cos, r = T.cos_rel(a, b)
        print(f"GENERAL {which} {what}: cosine {cos:.6f}, rel L2 {r:.3e}")
        if not (cos >= 0.999 and r <= 2e-2):
            failed.append(f"{what}: cosine {cos:.5f}, rel L2 {r:.3e}")
    assert not failed, failed
    # a clamped axis is exactly 0 on both sides
    lo, hi = aabb[:3], aabb[3:]
    clamped = (x <= lo) | (x >= hi)
    assert int(clamped.sum()) > 100 and not xg.grad.cpu()[clamped].any() and not xc.grad[clamped].any()


# ------------------------------------------------------------------------------------------------------------------------------- the ray level
RAY_COUNTS = (1, 63, 64, 65, 129)


def _ray_setup(dev, n, seed=3):
    import test_hip_ngp_train as T
    from dreg_nerf_amd import ngp_train, render
    f, g = T._block(dev, seed=seed)
    with torch.no_grad():
        f.aabb.copy_(torch.tensor(T.MODEL_INSIDE, dtype=torch.float32))
    rays = T._rays(n, seed=40 + n)
    dt = 0.02
    jitter = torch.rand(n, generator=torch.Generator().manual_seed(n)).to(dev)
    gen = torch.Generator().manual_seed(7 + n)
    ups = [torch.randn(n, 3, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)]
    return f.train(), g, rays, dt, jitter, ups, T, ngp_train, render


def _render_with_grads(f, g, rays, dt, jitter, ups, T, ngp_train, render, dev, inputs=True, params=True):
    o = rays.origins.to(dev).clone().requires_grad_(inputs)
    d = rays.viewdirs.to(dev).clone().requires_grad_(inputs)
    f.requires_grad_(params)
    f.mlp_base.params.grad = None
    f.color_mlp.params.grad = None
    rgb, op, dep, n_s = ngp_train.render_image_train(f, g, render.Rays(o, d), T.AABB, dt, torch.ones(3), jitter=jitter, backward="samples")
    loss = (rgb * ups[0]).sum() + (op[:, 0] * ups[1]).sum() + (dep[:, 0] * ups[2]).sum()
    loss.backward()
    f.requires_grad_(True)
    pg = (None, None) if not params else (f.mlp_base.params.grad.clone(), f.color_mlp.params.grad.clone())
    return (rgb.detach(), op.detach(), dep.detach()), (o.grad, d.grad), pg, n_s


@gpu
@pytest.mark.parametrize("n", RAY_COUNTS)
def test_ray_gradients_against_the_restatement(dev, n):
    """rays.origins.grad / rays.viewdirs.grad of render_image_train(backward="samples") equal the pieces called by hand (the list forward, the
    sort, dreg_ngp_samples_grad, dreg_ngp_points_input_grad, dreg_ngp_samples_ray_grad) bit for bit, and the ray kernel's sums equal
    ray_sums64 of the kernel's own per-sample gradients within (2 + n_r) 2^-24 M (one product and one sum per term, n_r terms)."""
    from dreg_nerf_amd import field_train as FT, render as R
    f, g, rays, dt, jitter, ups, T, ngp_train, render = _ray_setup(dev, n)
    outs, (go, gd), _, n_s = _render_with_grads(f, g, rays, dt, jitter, ups, T, ngp_train, render, dev)
    o, d = rays.origins.to(dev).contiguous(), rays.viewdirs.to(dev).contiguous()
    parts = R._grid_parts(g, dev)
    cap = ngp_train.default_sample_capacity(n, T.AABB, dt)
    rgb, op, dep, rec, count = ngp_train.render_train_samples(f, parts, o, d, jitter, T.AABB, dt, [1.0, 1.0, 1.0], 0.0, cap)
    assert count == n_s and (count > 0 or n == 1)
    srt = ngp_train.canonical_order(rec, count)
    grads = ngp_train.samples_grad(srt, d, rgb, op, dep, ups[0], ups[1], ups[2], dt)
    if grads is None:
        assert not go.any() and not gd.any()
        return
    gx, gdir = FT.points_input_grad(f, srt["x"], grads[0], grads[1], grads[2])
    go2, gd2 = ngp_train.samples_ray_grad(f, srt, grads, True, n)
    assert torch.equal(go, go2) and torch.equal(gd, gd2)
    want = IG.ray_sums64(srt["ray"].cpu().numpy(), srt["t"].cpu().numpy(), gx.cpu().numpy(), gdir.cpu().numpy(), n)
    bo, bd = (2 + want[4])[:, None] * U * want[1], (2 + 2 * want[4])[:, None] * U * want[3]
    eo, ed = np.abs(go.cpu().numpy() - want[0]), np.abs(gd.cpu().numpy() - want[2])
    assert np.all(eo <= bo) and np.all(ed <= bd)
    empty = want[4] == 0
    assert not go.cpu().numpy()[empty].any() and not gd.cpu().numpy()[empty].any()       # rays without survivors: zeros
    assert n == 1 or (go.abs().sum() > 0 and gd.abs().sum() > 0)
    r = float((eo[bo > 0] / bo[bo > 0]).max()) if (bo > 0).any() else 0.0
    print(f"RAY {n} rays, {count} samples: largest ratio dL/do {r:.3e}")


@gpu
def test_ray_gradients_deterministic_and_existing_outputs_unchanged(dev):
    """129 rays: dL/do and dL/dd bit-identical between two runs and between forward launch widths 1, 7 and 300; rgb, opacity, depth and the
    parameter gradients bit-identical with and without requires_grad on the inputs, also through field_points; with frozen parameters the ray
    gradients are the same and no parameter gradient is made."""
    from dreg_nerf_amd import field_train as FT, lib as L
    n = 129
    f, g, rays, dt, jitter, ups, T, ngp_train, render = _ray_setup(dev, n)
    args = (f, g, rays, dt, jitter, ups, T, ngp_train, render, dev)
    outs, (go, gd), (pb, pc), _ = _render_with_grads(*args)
    assert go.abs().sum() > 0 and gd.abs().sum() > 0
    with L.probe() as p:
        for waves in (2048, 1, 7, 300):
            p.set("dreg_render_samples_set_waves", waves, 2048)
            _, (go2, gd2), (pb2, pc2), _ = _render_with_grads(*args)
            assert torch.equal(go, go2) and torch.equal(gd, gd2), waves
            assert torch.equal(pb[:3072], pb2[:3072]) and torch.equal(pc, pc2), waves
    outs0, (no_o, no_d), (pb0, pc0), _ = _render_with_grads(*args, inputs=False)
    assert no_o is None and no_d is None
    assert all(torch.equal(a, b) for a, b in zip(outs, outs0)) and torch.equal(pb[:3072], pb0[:3072]) and torch.equal(pc, pc0)
    torch.testing.assert_close(pb[3072:], pb0[3072:], rtol=1e-4, atol=1e-5 * float(pb0[3072:].abs().max()))      # (the table: fp32 atomics)
    outs1, (go1, gd1), (pb1, pc1), _ = _render_with_grads(*args, params=False)
    assert pb1 is None and all(torch.equal(a, b) for a, b in zip(outs, outs1)) and torch.equal(go, go1) and torch.equal(gd, gd1)
    assert f.mlp_base.params.grad is None and f.color_mlp.params.grad is None
    with pytest.raises(ValueError):
        ngp_train.render_image_train(f, g, render.Rays(rays.origins.to(dev).requires_grad_(True), rays.viewdirs.to(dev)), T.AABB, dt, torch.ones(3))
    # field_points
    x, d = (torch.rand(300, 3, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev), rays.viewdirs[:1].to(dev).repeat(300, 1)
    res = []
    for req in (False, True):
        f.mlp_base.params.grad = None
        f.color_mlp.params.grad = None
        xs, ds = x.clone().requires_grad_(req), d.clone().requires_grad_(req)
        s, c = FT.field_points(f, xs, ds)
        (s.sum() + (c * c).sum()).backward()
        res.append((s.detach(), c.detach(), f.mlp_base.params.grad[:3072].clone(), f.color_mlp.params.grad.clone(), xs.grad, ds.grad))
    assert all(torch.equal(a, b) for a, b in zip(res[0][:4], res[1][:4]))
    assert res[0][4] is None and res[0][5] is None and res[1][4].abs().sum() > 0 and res[1][5].abs().sum() > 0


# ------------------------------------------------------------------------------------------------------------------------------ pose recovery
FIX_AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
FIX_DT = 0.02
FIX_H0_STD = 3.0                                         # of the density logit over the ball: opaque lumps in a thin medium
FIX_K = torch.tensor([[140.0, 0, 32.0], [0, 140.0, 24.0], [0, 0, 1]])      # the ball (radius 0.8 at distance 3.4) fills the 64 x 48 frame
FIX_W, FIX_H = 64, 48
POSE_ITERS, POSE_RAYS, POSE_LR = 30, 64, 5e-3            # few rays, a coarse step: the CPU arm costs about half a minute
START_TWIST = [0.02 * 0.2673, 0.02 * 0.5345, 0.02 * 0.8018 + 0.02, -0.0133, 0.0133, 0.0067]   # about 2 degrees about (1, 2, 3) + z, 0.02 of translation


def _look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    eye, target, up = torch.tensor(eye), torch.tensor(target), torch.tensor(up)
    back = torch.nn.functional.normalize(eye - target, dim=0)          # OpenGL: the camera looks down its -z
    right = torch.nn.functional.normalize(torch.linalg.cross(up, back), dim=0)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, torch.linalg.cross(back, right), back, eye
    return c2w


FIX_CAMS = torch.stack([_look_at(e) for e in ((2.6, -1.9, 1.2), (-2.2, 2.4, 0.8), (0.6, 2.9, -1.4), (-2.5, -1.6, -1.3))])


@functools.lru_cache(maxsize=None)
def fixture_block():
    """A block a pose can be recovered on, on the host: (field, grid).  tcnn's initial networks over a table whose DENSE coarse levels hold a
    smooth, non-symmetric function of the vertex position (a sine of a level- and feature-specific plane wave) and whose hashed fine levels are
    zero; row 0 of density W2 is rescaled so that the density logit has standard deviation FIX_H0_STD over the ball; a ball-shaped 32^3 occupancy grid of
    radius 0.8.  (The random tables of the other generated blocks are white noise in space and the constant table of
    tests/test_hip_field_train.py's _smooth_block has no spatial gradient: neither can move a pose.)"""
    from dreg_nerf_amd import ngp
    torch.manual_seed(77)
    f = ngp.NGPradianceField(FIX_AABB)
    rows, entries = N.level_table()
    gen = torch.Generator().manual_seed(78)
    table = torch.zeros(entries, 2)
    for row in rows:
        if row["hashed"]:
            continue
        res = row["res"]
        g = torch.arange(res, dtype=torch.float32)
        p = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        p = (p - 0.5) / row["scale"]                                     # the unit coordinates of the vertex
        idx = (p.new_tensor([1.0, res, res * res]) * torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)).sum(-1).long()
        for k in range(2):
            wave = (torch.rand(3, generator=gen) - 0.3) * 2.5
            table[row["offset"] + idx, k] = 0.5 * torch.sin(2 * math.pi * (p @ wave) + 6.28 * torch.rand(1, generator=gen))
    with torch.no_grad():
        f.mlp_base.params[3072:] = table.reshape(-1)
        x = torch.randn(4096, 3, generator=gen)
        x = x / x.norm(dim=1, keepdim=True) * 0.8 * torch.rand(4096, 1, generator=gen) ** (1 / 3)
        h0 = N.query_density(x, torch.tensor(FIX_AABB), f.mlp_base.params.detach())[1][:, 0]
        f.mlp_base.params[2048:2048 + 64] *= FIX_H0_STD / float(h0.std())
    grid = ngp.OccupancyGrid(FIX_AABB, 32)
    c = (torch.stack(torch.meshgrid(*[torch.arange(32)] * 3, indexing="ij"), -1).float() + 0.5) / 32 * 3.0 - 1.5
    grid._binary = c.norm(dim=-1) < 0.8
    return f.eval(), grid


def fixture_meta():
    return {"aabb_host": FIX_AABB, "render_step_size": FIX_DT, "alpha_thre": 0.0, "unbounded": False}


def oracle_render(field_cpu, grid_cpu):
    """The yardstick's differentiable render: render_train_restatement.march (under no_grad: t carries nothing), the oracle's field under the
    straight-through fp16 rounding, composite; on the CPU, whatever device the rays are on."""
    import render_train_restatement as RT
    base, color = field_cpu.mlp_base.params.detach().cpu(), field_cpu.color_mlp.params.detach().cpu()
    binary = grid_cpu.binary.cpu()
    aabb = torch.tensor(FIX_AABB)

    def render(block, rays):
        o, d = rays.origins.cpu(), rays.viewdirs.cpu()
        with torch.no_grad():
            tm, occ = RT.march(o.detach(), d.detach(), binary, aabb, aabb, FIX_DT, None)
        idx = torch.nonzero(occ)
        t_k = tm[idx[:, 0], idx[:, 1]]
        with RT.fp32_backward():
            x = o[idx[:, 0]] + t_k[:, None] * d[idx[:, 0]]
            sig, raw = N.query_density(x, aabb, base)
            col = N.query_rgb(d[idx[:, 0]], raw, color)
            sigma = torch.zeros(tm.shape).index_put((idx[:, 0], idx[:, 1]), sig)
            rgb_s = torch.zeros(*tm.shape, 3).index_put((idx[:, 0], idx[:, 1]), col)
            rgb, op, dep, surv = RT.composite(sigma, rgb_s, occ, tm, FIX_DT, torch.ones(3))
        return rgb, op, dep, int(surv.sum())
    return render


@gpu
def test_pose_recovery_against_autograd_as_the_yardstick(dev):
    """Source = target = the fixture block, ground truth the identity, start = Exp(START_TWIST) (about 2 degrees, 0.02).  Arm A:
    refine_pose_photometric (the kernel path).  Arm B: the same loop with the moving block's render and its gradient by torch autograd on the
    CPU through the oracle and composite (oracle_render), from the same start, three sampling seeds.  64 rays per direction at step 0.02 for 30
    iterations, lr 5e-3 (sized for the CPU arm, which is what this test costs: about 8 s per run; the sizes were chosen on arm B alone, which
    does not run the code under test).  Asserted first, as a condition on the inputs: every B run ends
    below half its starting rotation and translation error.  Then A's final RRE and RTE <= the worst B x (1 + s), s = B's own seed-to-seed
    spread (max / min - 1), per metric."""
    from dreg_nerf_amd import photo_refine as PR
    f_cpu, g_cpu = fixture_block()
    import copy
    f_dev, g_dev = copy.deepcopy(f_cpu).to(dev).eval(), copy.deepcopy(g_cpu).to(dev)
    g_dev._binary = g_cpu.binary.to(dev)
    block = (f_dev, g_dev, fixture_meta())
    start = PR.se3_exp(torch.tensor(START_TWIST, dtype=torch.float64))
    gt = torch.eye(4, dtype=torch.float64)
    r0, t0 = PR.pose_errors(start, gt)
    assert 1.5 < r0 < 3.0 and 0.015 < t0 < 0.03
    kw = dict(iters=POSE_ITERS, n_rays=POSE_RAYS, lr=POSE_LR, depth_weight=0.1, symmetric=True)
    b = []
    for seed in (1, 2, 3):
        pose, info = PR.refine_pose_photometric(block, block, start, FIX_CAMS, FIX_CAMS, FIX_K, FIX_W, FIX_H, seed=seed,
                                                moving_render=oracle_render(f_cpu, g_cpu), **kw)
        b.append(PR.pose_errors(pose, gt))
        assert info["skipped"] == 0
    print(f"arm B (autograd, CPU): start RRE {r0:.3f} deg, RTE {t0:.4f} -> {[(round(r, 3), round(t, 4)) for r, t in b]}")
    assert all(r < 0.5 * r0 and t < 0.5 * t0 for r, t in b), (r0, t0, b)             # the condition on the inputs
    pose, info = PR.refine_pose_photometric(block, block, start, FIX_CAMS, FIX_CAMS, FIX_K, FIX_W, FIX_H, seed=1, **kw)
    ra, ta = PR.pose_errors(pose, gt)
    sr = max(r for r, _ in b) / min(r for r, _ in b) - 1.0
    st = max(t for _, t in b) / min(t for _, t in b) - 1.0
    print(f"arm A (kernel): RRE {ra:.3f} deg, RTE {ta:.4f}; worst B {max(r for r, _ in b):.3f} / {max(t for _, t in b):.4f}, spreads {sr:.3f} / {st:.3f}; "
          f"loss {info['loss'][0]:.5f} -> {info['loss'][-1]:.5f}, masks {info['mask'][0]} -> {info['mask'][-1]}, samples {info['samples'][-1]}")
    assert all(p.requires_grad for p in (f_dev.mlp_base.params, f_dev.color_mlp.params))      # the freeze is undone
    assert ra <= max(r for r, _ in b) * (1.0 + sr) and ta <= max(t for _, t in b) * (1.0 + st), (ra, ta, b)


# ------------------------------------------------------------------------------------------------------------------------------- the product
@gpu
def test_photo_refine_product_through_main(dev, tmp_path, monkeypatch, capsys):
    """eval_nerf_regtr.py's main() on the generated three-block tree of tests/test_hip_scene_grid.py with --photo_refine at 3 iterations of 256
    rays (untrained weights: plumbing): photo_refined_metrics_test.json exists with icp.write_refined_metrics' schema plus the start errors and
    the iterations; metrics_test.json is byte-equal to a run without the flag (but for the host clock around the forward call)."""
    import test_hip_pair_field as TPF
    import test_hip_render_pair as TP
    import test_hip_render_scene as TS
    import test_hip_scene_grid as TG
    from dreg_nerf_amd import render as R
    monkeypatch.setitem(R.INTRINSICS, "objaverse", (TP.W, TP.H, 60.0, 60.0, 32.0, 24.0))
    four = [TP._block(seed, shell=shell) for seed, shell in TS.SHELLS]
    root, jd = tmp_path / "data", tmp_path / "json"
    TG._three_block_tree(four, root, jd)
    common = ["--root_dir", str(root), "--json_dir", str(jd), "--dataset", "objaverse", "--precision", "fp32"]
    TS._main(monkeypatch, common + ["--expname", "plain"])
    TS._main(monkeypatch, common + ["--expname", "photo", "--photo_refine", "--photo_iters", "3", "--photo_rays", "256"])
    text = capsys.readouterr().out
    assert "sceneA: photometric refinement, 3 iterations" in text and "photometric refinement, 1 scenes" in text
    base = lambda name: str(root / "eval" / name / "objaverse")
    assert TPF._without_time(os.path.join(base("photo"), "metrics_test.json")) == TPF._without_time(os.path.join(base("plain"), "metrics_test.json"))
    assert not os.path.exists(os.path.join(base("plain"), "photo_refined_metrics_test.json"))
    out = json.load(open(os.path.join(base("photo"), "photo_refined_metrics_test.json")))
    row = out["sceneA"]
    assert set(row) == {"R_mean", "t_mean", "R_med", "t_med", "time", "R_start", "t_start", "iterations", "skipped"} and row["iterations"] == 3
    assert out["R_mean"] == row["R_mean"] and out["t_mean"] == row["t_mean"] and all(math.isfinite(float(v)) for v in row.values())
    plain = json.load(open(os.path.join(base("plain"), "metrics_test.json")))
    assert abs(row["R_start"] - plain["sceneA"]["R_mean"]) < 1e-3 and abs(row["t_start"] - plain["sceneA"]["t_mean"]) < 1e-4      # it starts from the predicted pose
