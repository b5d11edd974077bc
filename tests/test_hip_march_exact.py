"""GPU: the ray marchers (csrc/march.h through render.hip, its training form, and visibility.hip in all its forms) against the fp64 march of
tests/march_restatement.py, ray by ray.

The field has a zeroed hash table and no bias: the density logit is exactly 0 and sigma = exp(-1) at every sample strictly inside the model
aabb, 0 outside it.  A sample's alpha is then one constant a, measured from a ray that keeps one sample (test_calibration), and a rendered ray
is a closed form of the SET OF LATTICE SAMPLES IT KEPT:
  opacity = 1 - q^n  (q = fl32(1 - a), n = kept samples inside the model aabb)   -> n = round(log1p(-opacity) / log(q))
  depth   = sum_j a q^j t_j                                                       -> which samples
  rgb     = c(d) opacity + bkgd (1 - opacity), c = the colour net on zero features (oracle.ngp_oracle.query_rgb), within 4e-3
  label   = "some kept in-model sample lies in front of the point" at cut_off = a / 2, alpha_thre = 0.
The input sets are tests/march_cases.py; tests/test_march_host.py asserts on the CPU that at most 2 % of the rays of each random set are
undecidable (tests/march_restatement.py: a rounding could change the kept set) and that n a <= 2 (no ray ends early).

Depth tolerance: 4 x the largest difference, over the rays of the input set, between the closed form accumulated in fp32 in the kernel's order
(fp32 t_min, t = fl(t_min + fl((n + 1/2) dt)), T *= q, depth += fl(fl(a T) t)) and in fp64, both at the kernel's own alpha (the roundings of
T *= q depend on the bits of q) — of the order n 2^-23 depth.  Measured (Case.depth_fp32_error) over alphas within 4 * 2^-24 of the fp64 value: largest
difference 1.8e-7 over the random sets (ragged grid, dt 0.02, n <= 46; 7.3e-8 at dt 0.005, 4.3e-9 at dt 1e-3) and between 1.5e-7 and 8.1e-7 over the
exact cases (n <= 256; 6.2e-7 at the alpha an MI355X returns, where the kernel's depth equals the fp32 run to the last bit), so the tolerances lie
between 2e-9 (random 10 % grid, dt 1e-3) and 3.2e-6, absolute.  One sample moved by one lattice step changes the depth by a (1 - a)^n dt >= 3.5e-7
at dt 1e-3, 7.7e-6 at dt 0.005, 1.0e-4 at dt 0.02 and 2.0e-5 in the exact cases: at least 4 x the tolerance of its set for every compared ray
(asserted here at the kernel's alpha, and in tests/test_march_host.py at the fp64 one)."""
import math

import numpy as np
import pytest
import torch

import march_cases as C
from dreg_nerf_amd import ngp, ngp_train, visibility
from dreg_nerf_amd import render as R
from oracle import ngp_oracle as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BK = torch.tensor(C.BKGD)


@pytest.fixture(scope="module")
def field():
    g = torch.Generator().manual_seed(21)
    f = ngp.NGPradianceField(C.EXACT_MODEL)
    with torch.no_grad():
        f.mlp_base.params[:3072] = torch.randn(3072, generator=g)
        f.mlp_base.params[3072:] = 0.0                               # every hash-grid feature is 0: the density logit is exactly 0
        f.color_mlp.params.copy_(torch.randn(7168, generator=g) * 0.2)
    return f.to(DEV).eval()


def _with_model(f, model):
    with torch.no_grad():
        f.aabb.copy_(torch.tensor(model, dtype=torch.float32))
    return f


def _grid(case, coarse="true"):
    b8 = torch.from_numpy(case.binary).to(DEV).to(torch.uint8).contiguous()
    bits = visibility.coarse_occupancy_bits(b8)
    if coarse == "all":
        bits = torch.full_like(bits, -1)                             # no empty 4^3 block: every cell is looked up on its own
    return R.BlockGrid(case.roi, b8, bits)


def _render(f, case, coarse="true"):
    _with_model(f, case.model)
    rays = R.Rays(torch.from_numpy(case.o).to(DEV), torch.from_numpy(case.d).to(DEV))
    with torch.no_grad():
        if case.jitter is not None:
            rgb, op, dep, ns = ngp_train.render_image_train(f, _grid(case, coarse), rays, case.scene, case.dt, render_bkgd=BK,
                                                            jitter=torch.from_numpy(case.jitter).to(DEV))
        else:
            rgb, op, dep, ns = R.render_image(f, _grid(case, coarse), rays, case.scene, near_plane=case.near, far_plane=case.far,
                                              render_step_size=case.dt, render_bkgd=BK)
    return rgb.cpu().double().numpy(), op.reshape(-1).cpu().double().numpy(), dep.reshape(-1).cpu().double().numpy(), ns


_A = {}


def _a_gpu(f, dt):
    """The kernel's alpha at step dt: the opacity of a ray that keeps exactly one sample."""
    if dt not in _A:
        c = C.calibration_case(dt)
        assert c.ref.n_kept.tolist() == [1]
        _A[dt] = float(_render(f, c)[1][0])
    return _A[dt]


@pytest.mark.parametrize("dt", (C.EXACT_DT,) + C.RANDOM_DTS)
def test_calibration(field, dt):
    a = _a_gpu(field, float(np.float32(dt)))
    print(f"dt {dt}: a_gpu {a!r}, a_fp64 {C.alpha64(dt)!r}, difference {a - C.alpha64(dt):.3e}")
    assert abs(a - C.alpha64(dt)) <= 4 * 2.0 ** -24                  # a = 1 - exp(..): the subtraction is from 1, so the bound is absolute


def _check(f, case, out, sel, rgb_check=True):
    """Rays `sel` of a launch against the fp64 march: decoded n, depth, rgb."""
    rgb, op, dep, _ = out
    r = case.ref
    a = _a_gpu(f, case.dt)
    q = float(np.float32(1) - np.float32(a))
    n_dec = np.round(np.log1p(-op) / math.log(q)).astype(np.int64)
    op_ref, dep_ref = r.composite(a, q)
    tol = case.depth_tolerance(a)                                    # the fp32 run of the SAME closed form: the kernel's alpha
    sens = case.step_sensitivity()
    bad_n = sel & (n_dec != r.n_model)
    ddiff = np.abs(dep - dep_ref)
    print(f"{case.name}: {int(sel.sum())} rays compared of {len(sel)}, {int((r.n_kept[sel] > 0).sum())} keep samples (max n {int(r.n_model[sel].max())}); wrong n on {int(bad_n.sum())}; "
          f"largest depth difference {ddiff[sel].max():.3e} (tolerance {tol:.3e}, smallest one-step change {sens[sel].min():.3e})")
    assert r.n_model[sel].max() * a <= 2.0
    assert not bad_n.any(), [(int(i), int(n_dec[i]), int(r.n_model[i])) for i in np.nonzero(bad_n)[0][:10]]
    assert (sens[sel] >= 4 * tol).all()
    assert (ddiff[sel] <= tol).all(), [(int(i), dep[i], dep_ref[i]) for i in np.nonzero(sel & (ddiff > tol))[0][:10]]
    if rgb_check:
        col = N.query_rgb(torch.from_numpy(case.d), torch.zeros(len(case.d), 16), f.color_mlp.params.detach().cpu()).double().numpy()
        want = col * op_ref[:, None] + np.array(C.BKGD) * (1.0 - op_ref[:, None])
        cdiff = np.abs(rgb - want).max(axis=1)
        print(f"{case.name}: largest rgb difference {cdiff[sel].max():.3e}")
        assert (cdiff[sel] <= 4e-3).all()


@pytest.mark.parametrize("grid", sorted(C.EXACT_GRIDS))
@pytest.mark.parametrize("planes", sorted(C.EXACT_PLANES))
def test_exact_cases(field, grid, planes):
    """Dyadic inputs: fp32 evaluates the rule without rounding, with or without fma.  EVERY ray is compared."""
    for pattern in C.EXACT_PATTERNS:
        case = C.exact_case(grid, planes, pattern)
        r = case.ref
        out = _render(field, case)
        every = np.ones(len(case.o), bool)
        _check(field, case, out, every, rgb_check=False)
        rgb, op, dep, ns = out
        none = r.n_kept == 0                                         # missed rays, empty intervals, rays through empty cells: exactly (bkgd, 0, 0)
        assert none.any()
        assert np.array_equal(rgb[none], np.broadcast_to(np.array(C.BKGD, np.float32).astype(np.float64), (int(none.sum()), 3)))
        assert not op[none].any() and not dep[none].any()
        assert ns == int(r.n_kept.sum()), (pattern, ns, int(r.n_kept.sum()))


@pytest.mark.parametrize("grid", C.RANDOM_GRIDS)
@pytest.mark.parametrize("dt", C.RANDOM_DTS)
def test_random_and_grazing_rays(field, grid, dt):
    case = C.random_case(grid, dt)
    r = case.ref
    out = _render(field, case)
    _check(field, case, out, r.decidable)
    # coarse bits change nothing: the same fp32 arithmetic on both sides, so ALL rays are compared, bit for bit
    out_all = _render(field, case, coarse="all")
    for x, y, what in zip(out[:3], out_all[:3], ("rgb", "opacity", "depth")):
        assert np.array_equal(x, y), (what, np.nonzero((x != y).reshape(len(case.o), -1).any(axis=1))[0][:10])
    assert out[3] == out_all[3]


def test_coarse_bits_change_nothing_for_grazing_rays_at_the_default_step(field):
    """20,000 nearly axis-parallel rays through a 128^3 shell at dt = 1e-3 with the true coarse bits and with all bits set: equal outputs on
    every ray.  Both launches still skip (a block there, a cell here), so 3,000 of the rays are also compared with the rule evaluated in fp32
    at EVERY lattice point (Case.stepped_fp32: the kernels use no fused multiply-add and correctly rounded division, so the samples are the
    same on every ray, no margin): the skip's allowance of 1e-3 of a step, which march_steps_to_face replaces, passed over occupied lattice
    points next to a block's exit face on such rays (a host copy of that loop loses two samples on ray 7217)."""
    b, aabb, o, d = C.coarse_rays()
    case = C.Case("coarse-grazing", b, aabb, aabb, aabb, o, d, 1e-3)
    a = _render(field, case)
    c = _render(field, case, coarse="all")
    diff = (a[1] != c[1]) | (a[2] != c[2]) | (a[0] != c[0]).any(axis=1)
    print(f"coarse-grazing: {int(diff.sum())} of {len(o)} rays differ, surviving samples {a[3]} / {c[3]}")
    sl = C.STEPPED_SLICE
    kept, n_model = C.Case("coarse-grazing-slice", b, aabb, aabb, aabb, o[sl], d[sl], 1e-3).stepped_fp32()
    al = _a_gpu(field, case.dt)
    assert n_model.max() * al <= 2.0 and n_model.max() * 2.0 ** -24 / al < 0.5
    n_dec = np.round(np.log1p(-a[1][sl]) / math.log(float(np.float32(1) - np.float32(al)))).astype(np.int64)
    wrong = np.nonzero(n_dec != n_model)[0]
    print(f"coarse-grazing: decoded n differs from the fp32 stepping on {len(wrong)} of {len(n_dec)} rays: {[(int(i) + sl.start, int(n_dec[i]), int(n_model[i])) for i in wrong[:10]]}")
    assert not diff.any(), np.nonzero(diff)[0][:10]
    assert a[3] == c[3] and a[3] > 1000000
    assert len(wrong) == 0


@pytest.mark.parametrize("jitter", C.JITTERS, ids=[str(j) for j in C.JITTERS])
def test_training_forward_with_jitter(field, jitter):
    """dreg_ngp_render_train: the lattice starts at t_min + u dt, u per ray — 0, 1/2, the largest fp32 below 1, random."""
    case = C.train_case(jitter)
    out = _render(field, case)
    _check(field, case, out, case.ref.decidable)
    if jitter == 0.0:                                                # u = 0 is the inference kernel, bit for bit
        plain = _render(field, C.random_case("ragged", 0.005))
        assert all(np.array_equal(x, y) for x, y in zip(out[:3], plain[:3])) and out[3] == plain[3]


def _labels(f, v, persistent, coarse):
    pts, cams = torch.from_numpy(v.pts).to(DEV), torch.from_numpy(v.cams).to(DEV)
    b = torch.from_numpy(v.binary).to(DEV)
    visibility.PERSISTENT, visibility.COARSE = persistent, coarse
    return visibility.surface_visibility(pts, cams, f, b, v.roi, v.scene, v.dt, cut_off=v.cut_off, alpha_thre=0.0).cpu().numpy()


@pytest.mark.parametrize("distinct", [True, False], ids=["three_aabbs", "roi_is_scene"])
def test_visibility_labels(field, distinct, tmp_path):
    """Lock-step, persistent without and with coarse bits (and, where roi == scene as that entry point has it, the batched launch over a
    checkpoint): equal to the fp64 labels on decidable points, equal to each other on ALL points."""
    v = C.vis_case(distinct)
    lab, dec, _ = v.ref
    _with_model(field, v.model)
    labs = {}
    try:
        for persistent, coarse in ((False, False), (True, False), (True, True)):
            labs[(persistent, coarse)] = _labels(field, v, persistent, coarse)
        if not distinct:
            poses = torch.eye(4)[None].repeat(len(v.cams), 1, 1)
            poses[:, :3, 3] = torch.from_numpy(v.cams)
            occ = ngp.OccupancyGrid(v.roi, list(v.binary.shape))
            occ._binary.copy_(torch.from_numpy(v.binary))
            path = str(tmp_path / "block.pth")
            torch.save({"step": 1, "model": field.state_dict(), "occupancy_grid": occ.state_dict(), "aabb": v.roi, "unbounded": False,
                        "near_plane": None, "far_plane": None, "grid_resolution": list(v.binary.shape), "contraction_type": ngp.ContractionType.AABB,
                        "render_step_size": v.dt, "alpha_thre": 0.0, "cone_angle": 0.0, "camera_poses": poses, "block_id": 0}, path)
            visibility.clear_block_cache()
            visibility.PERSISTENT = visibility.COARSE = True
            got = visibility.compute_visibility_scores_batched([(torch.from_numpy(v.pts).to(DEV)[None], path)], cut_off=v.cut_off)[0]
            labs["batched"] = got.reshape(-1).cpu().numpy() > 0
            visibility.clear_block_cache()
    finally:
        visibility.PERSISTENT = visibility.COARSE = True
    visibility.OVERRUN.check(wait=True)
    for k, g in labs.items():
        wrong = dec & (g != lab)
        print(f"{v.name} {k}: {int(g.sum())} of {len(g)} labelled (reference {int(lab.sum())}), wrong on {int(wrong.sum())} of {int(dec.sum())} decidable points")
    for k, g in labs.items():
        assert not (dec & (g != lab)).any(), (k, np.nonzero(dec & (g != lab))[0][:10])
    ref = labs[(False, False)]
    for k, g in labs.items():
        assert np.array_equal(g, ref), (k, np.nonzero(g != ref)[0][:10])
    assert 0 < int(lab.sum()) < len(lab)
