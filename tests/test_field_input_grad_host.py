"""CPU: the fp64 restatement of the field's input gradients (tests/field_input_grad_restatement.py) against torch autograd on a
general field and through the march and the compositing; its known answers; the planted errors against the GPU test's bound; the argument guards
of dreg_ngp_points_input_grad and dreg_ngp_samples_ray_grad; the raises and flags of the host side (ngp_train, field_train, photo_refine,
eval_nerf_regtr.py)."""
import ctypes
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
import render_samples_restatement as RS
import render_train_restatement as RT
import test_hip_field_input_grad as G
from oracle import ngp_oracle as N


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _general(seed=3):
    gen = torch.Generator().manual_seed(seed)
    base = torch.empty(3072 + N.n_grid_params()).uniform_(-0.5, 0.5, generator=gen)
    base[:3072].uniform_(-0.3, 0.3, generator=gen)
    color = torch.empty(7168).uniform_(-0.3, 0.3, generator=gen)
    return gen, base, color, torch.tensor([-0.6, -0.55, -0.65, 0.55, 0.6, 0.5])


def test_sh4_monomials_are_the_oracles_polynomials():
    d = torch.randn(200, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    assert np.abs(IG.sh4_value(d.numpy()) - N.sh4(d).numpy()).max() < 1e-14
    J = IG.sh4_jacobian(d.float().numpy())[0]
    dd = d.float().double().requires_grad_(True)
    for j in (4, 9, 12, 15):
        (g,) = torch.autograd.grad(N.sh4(dd)[:, j].sum(), dd)
        assert np.abs(J[:, j] - g.numpy()).max() < 1e-13


@pytest.mark.parametrize("which", ["sigma", "rgb", "both"])
def test_restatement_equals_autograd_on_a_general_field(which):
    """input_grad64, fed the oracle's own forward record of a random non-flat field, against autograd through oracle.ngp_oracle.query_density /
    query_rgb with x and dirs requiring grad, under fp32_backward(): relative L2 <= 1e-4 over the whole [N,3] arrays (§3m's and §3o's bound for
    the same comparison).  Autograd differentiates the sigmoid at its unrounded value s: the record's c is s here."""
    gen, base, color, aabb = _general()
    n = 1500
    x = ((torch.rand(n, 3, generator=gen) - 0.5) * 1.6).requires_grad_(True)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1).requires_grad_(True)
    gs = torch.randn(n, generator=gen) * (which != "rgb")
    gc = torch.randn(n, 3, generator=gen) * (which != "sigma")
    with RT.fp32_backward():
        sig, raw = N.query_density(x, aabb, base)
        rgb = N.query_rgb(d, raw, color)
        ((sig * gs).sum() + (rgb * gc).sum()).backward()
    record, weights, inside = FP.forward_record(x.detach(), d.detach(), base, color, aabb)
    assert 100 < int((~inside).sum()) < n - 100
    record["c"] = record["s"]
    res = IG.input_grad64(record, weights, N.f16(base[3072:]).numpy().reshape(-1, 2), d.detach().numpy(), gs.numpy() if which != "rgb" else None,
                          gc.numpy() if which != "sigma" else None, B.levels(), aabb.tolist())
    assert np.array_equal(res.inside, inside)
    r = _rel(res.gx, x.grad.double().numpy())
    print(f"restatement vs autograd ({which}), dL/dx: rel L2 {r:.3e}")
    assert r <= 1e-4, r
    assert not res.gx[~res.open].any() and not x.grad.numpy()[~res.open].any()              # a clamped axis: exactly 0 on both sides
    if which == "sigma":
        assert not res.gd.any() and not d.grad.any()
    else:
        r = _rel(res.gd, d.grad.double().numpy())
        print(f"restatement vs autograd ({which}), dL/ddir: rel L2 {r:.3e}")
        assert r <= 1e-4, r
        out1 = (~res.open).sum(1) == 1                                                      # outside on one axis: the other two keep the colour term
        assert out1.sum() > 50 and np.all((res.gx[out1] != 0).sum(1) == 2)


def test_ray_sums_against_autograd_through_march_and_composite():
    """dL/do, dL/dd of a colour + opacity + depth loss: autograd through x = o + t d (t from render_train_restatement.march under no_grad, so it
    carries nothing), the oracle's field and composite, against sample_grads64 -> input_grad64 -> ray_sums64 on the survivors: <= 1e-4."""
    gen, base, color, aabb = _general(5)
    base = base.clone()
    base[2048:2048 + 64] *= 0.2                                          # (moderate densities: rays keep many survivors)
    R, dt = 48, 0.05
    scene = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    c = (torch.stack(torch.meshgrid(*[torch.arange(16)] * 3, indexing="ij"), -1).float() + 0.5) / 16 * 2.0 - 1.0
    binary = c.norm(dim=-1) < 0.8
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1) * 2.5
    d = torch.nn.functional.normalize((torch.rand(R, 3, generator=gen) - 0.5) * 0.8 - o, dim=-1)
    d[-2:] = torch.nn.functional.normalize(o[-2:], dim=-1)              # two rays that look away: no survivors
    jitter = torch.rand(R, generator=gen)
    bk =torch.tensor([1.0, 0.5, 0.25])
    with torch.no_grad():
        tm, occ = RT.march(o, d, binary, scene, scene, dt, jitter)
    idx = torch.nonzero(occ)
    o.requires_grad_(True)
    d.requires_grad_(True)
    t_k = tm[idx[:, 0], idx[:, 1]]
    with RT.fp32_backward():
        x = o[idx[:, 0]] + t_k[:, None] * d[idx[:, 0]]
        sig, raw = N.query_density(x, aabb, base)
        col = N.query_rgb(d[idx[:, 0]], raw, color)
        S = tm.shape[1]
        sigma = torch.zeros(R, S).index_put((idx[:, 0], idx[:, 1]), sig)
        rgb_s = torch.zeros(R, S, 3).index_put((idx[:, 0], idx[:, 1]), col)
        rgb, opac, depth, surv = RT.composite(sigma, rgb_s, occ, tm, dt, bk)
        g_C, g_O, g_D = torch.randn(R, 3, generator=gen), torch.randn(R, generator=gen), torch.randn(R, generator=gen)
        ((rgb * g_C).sum() + (opac * g_O).sum() + (depth * g_D).sum()).backward()
    record, weights, inside = FP.forward_record(x.detach(), d.detach()[idx[:, 0]], base, color, aabb)
    alpha = 1.0 - np.exp(-sig.detach().double().numpy() * float(np.float32(dt)))
    rec = RS.records64(idx[:, 0].numpy(), t_k.numpy(), alpha, record["s"], bk.numpy(), R)
    assert np.array_equal(rec.surv, surv[idx[:, 0], idx[:, 1]].numpy()) and 200 < len(rec.kept) and (~inside[rec.kept]).any()
    g_sigma, g_c, _, _ = RS.sample_grads64(rec, g_C.numpy(), g_O.numpy(), g_D.numpy(), dt)
    k = rec.kept
    sub = {key: v[k] for key, v in record.items()}
    sub["c"] = sub["s"]
    dirs = d.detach().numpy()[rec.ray]
    res = IG.input_grad64(sub, weights, N.f16(base[3072:]).numpy().reshape(-1, 2), dirs, g_sigma, g_c, B.levels(), aabb.tolist())
    go, _, gd, _, cnt = IG.ray_sums64(rec.ray, rec.t, res.gx, res.gd, R)
    ro, rd = _rel(go, o.grad.double().numpy()), _rel(gd, d.grad.double().numpy())
    print(f"ray sums vs autograd: dL/do rel L2 {ro:.3e}, dL/dd rel L2 {rd:.3e} over {len(k)} survivors of {R} rays")
    assert ro <= 1e-4 and rd <= 1e-4, (ro, rd)
    assert (cnt == 0).any() and not go[cnt == 0].any() and not o.grad.numpy()[cnt == 0].any()      # rays without survivors get zeros
    bad = IG.ray_sums64(rec.ray, rec.t, res.gx, res.gd, R, mutate="t_next")
    assert _rel(bad[2], d.grad.double().numpy()) > 1e-3


# --------------------------------------------------------------------------------------------------------------------------------- known answers
def test_affine_level_zero_gives_a_position_independent_encoding_jacobian():
    """Dense level 0 holding (a ix + b iy + c iz) / 64 in feature 0 and zeros elsewhere: d enc_0 / du = scale_0 (a, b, c) / 64 inside every cell,
    every other column 0, and dL/dx = de_0 scale_0 (a, b, c) / 64 / (hi - lo)."""
    lv = B.levels()
    rows, entries = N.level_table()
    assert not rows[0]["hashed"] and rows[0]["res"] == 16
    a, b, c = 1.0, 2.0, 3.0
    table = np.zeros((entries, 2), np.float32)
    ix, iy, iz = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    table[(ix + 16 * iy + 256 * iz).ravel(), 0] = ((a * ix + b * iy + c * iz) / 64.0).ravel()
    assert np.array_equal(table.astype(np.float16).astype(np.float32), table)
    u = (0.05 + 0.85 * np.random.default_rng(0).random((500, 3))).astype(np.float32)       # (below the last vertex row, where the dense index wraps)
    E, _ = IG.encoding_jacobian(u, table, lv)
    want = float(lv["scale"][0]) * np.array([a, b, c]) / 64.0
    assert np.abs(E[:, 0, :] - want).max() < 1e-12 and not E[:, 1:, :].any()
    # through the whole rule
    gen, base, color, aabb = _general(9)
    base = base.clone()
    base[3072:] = torch.from_numpy(table.ravel())
    lo, hi = aabb[:3].numpy(), aabb[3:].numpy()
    x = (lo + u[:64] * (hi - lo)).astype(np.float32)
    d = torch.nn.functional.normalize(torch.randn(64, 3, generator=gen), dim=-1)
    record, weights, inside = FP.forward_record(x, d, base, color, aabb)
    assert inside.all()
    res = IG.input_grad64(record, weights, table, d.numpy(), np.ones(64), np.ones((64, 3)), lv, aabb.tolist())
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    assert np.abs(res.gx - res.de[:, :1] * want[None] / ext[None]).max() <= 1e-12 * np.abs(res.gx).max() and np.abs(res.gx).min() > 0


def test_clamped_axis_and_outside_known_answers():
    gen, base, color, aabb = _general(11)
    x = np.array([[0.0, 0.1, 0.2], [0.7, 0.1, 0.2], [0.0, -0.9, 0.9], [0.55, 0.1, 0.2]], np.float32)      # inside; out on x; out on y and z; ON the face
    d = torch.nn.functional.normalize(torch.randn(4, 3, generator=gen), dim=-1)
    record, weights, inside = FP.forward_record(x, d, base, color, aabb)
    table = N.f16(base[3072:]).numpy().reshape(-1, 2)
    both = IG.input_grad64(record, weights, table, d.numpy(), np.ones(4), np.ones((4, 3)), B.levels(), aabb.tolist())
    assert both.inside.tolist() == [True, False, False, False]
    assert np.all(both.gx[0] != 0)
    assert both.gx[1, 0] == 0 and np.all(both.gx[1, 1:] != 0)                               # the colour term stays on the other two axes
    assert both.gx[2, 0] != 0 and not both.gx[2, 1:].any()
    assert both.gx[3, 0] == 0 and np.all(both.gx[3, 1:] != 0)                               # u_c == 1 is not strictly inside
    sig = IG.input_grad64(record, weights, table, d.numpy(), np.ones(4), None, B.levels(), aabb.tolist())
    assert np.all(sig.gx[0] != 0) and not sig.gx[1:].any() and not sig.de[1:].any() and not sig.gd.any()      # dL/dh0 is off outside the aabb


# --------------------------------------------------------------------------------------------------------------------------------- planted errors
def test_planted_cases_are_what_the_gpu_test_needs():
    for n in G.EDGE_COUNTS:
        c = G.plant_case(n)
        assert set(np.nonzero(c.g_sigma)[0]) == set(c.hits) == set(np.nonzero(c.g_rgb.any(1))[0])
        assert set(c.hits) == {p for p in G.HIT_LANES + (n - 1,) if p < n}
        res, rec, margin = G.plant_reference(c)
        assert margin.min() >= 2 * G.GATE_MARGIN
        lo, hi = np.array(G.MODEL[:3], np.float32), np.array(G.MODEL[3:], np.float32)
        out_axes = (~((c.x[c.hits] > lo) & (c.x[c.hits] < hi))).sum(1)
        assert out_axes.tolist() == [(0, 1, 3)[k] for k in c.kind] and np.array_equal(res.inside, c.kind == 0)
        assert np.all(np.abs(res.gx[c.kind == 0]) > 0) and np.all(np.abs(res.gd) > 0)
    t = G.plant_table()
    assert np.unique(t[:4096]).size > 1000                                                 # not constant across corners


@pytest.mark.parametrize("mutate", IG.MUTATIONS)
def test_every_mutation_is_seen(mutate):
    """Each planted error moves an element of the 129-point case beyond four times the bound the GPU test holds the kernel to (§3m's criterion;
    the ray-sum error: beyond the ray test's bound on a list made of the case's hits).  The factor is printed per mutation; the smallest of
    the seven is DESIGN.md §3p's figure.  The dropped corner is corner 7 of the finest level, as in §3m: the bound scales with the sum of the
    absolute terms of ALL levels, which the fine levels dominate (scale_15 / scale_0 = 273), so one corner of level 0 stays inside it."""
    c = G.plant_case(129)
    res, rec, _ = G.plant_reference(c)
    bx, bd = G.bounds(res, rec["raw"][:, 0])
    if mutate == "t_next":
        ray, t = np.array([0, 0, 0, 2, 2, 2]), np.array([0.5, 0.75, 1.25, 0.25, 0.5, 2.0], np.float32)
        good, bad = IG.ray_sums64(ray, t, res.gx, res.gd, 3), IG.ray_sums64(ray, t, res.gx, res.gd, 3, mutate=mutate)
        bound = (2 + 2 * good[4])[:, None] * G.U * good[3]
        diff = np.abs(bad[2] - good[2])
        assert not np.abs(bad[0] - good[0]).any()
    else:
        bad, _, _ = G.plant_reference(c, mutate=mutate)
        diff, bound = np.concatenate([np.abs(bad.gx - res.gx), np.abs(bad.gd - res.gd)], 1), np.concatenate([bx, bd], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    worst = float(ratio.max())
    print(f"{mutate}: {worst:.3g} x the bound")
    assert worst > 4.0


# --------------------------------------------------------------------------------------------------------------------------- the entries' guards
EINVAL = -1
DEV = 0x10000                 # stands for a device buffer: the entry points read through none of them on the host
_u16 = (ctypes.c_uint32 * 16)(*range(16))
_f16 = (ctypes.c_float * 16)(*[1.0] * 16)
LEVELS = [ctypes.addressof(_u16)] * 3 + [ctypes.addressof(_f16), ctypes.addressof(_u16)]


def _call(n=1, aabb=(0, 0, 0, 1, 1, 1), **over):
    from dreg_nerf_amd import lib as L
    lib = L.load()
    box = (ctypes.c_float * 6)(*aabb) if aabb is not None else None           # (kept alive until the call returns)
    a = dict(x=DEV, dirs=DEV, base16=DEV, color16=DEV, offset=LEVELS[0], size=LEVELS[1], res=LEVELS[2], scale=LEVELS[3], hashed=LEVELS[4],
             aabb=ctypes.addressof(box) if box is not None else None, g_sigma=DEV, g_rgb=DEV, grad_x=DEV, grad_dir=DEV)
    a.update(over)
    return lib.dreg_ngp_points_input_grad(a["x"], a["dirs"], n, a["base16"], a["color16"], a["offset"], a["size"], a["res"], a["scale"], a["hashed"],
                                          a["aabb"], a["g_sigma"], a["g_rgb"], a["grad_x"], a["grad_dir"], None)


BAD = [dict(x=None), dict(dirs=None), dict(base16=None), dict(color16=None), dict(offset=None), dict(size=None), dict(res=None), dict(scale=None),
       dict(hashed=None), dict(aabb=None), dict(aabb=(0, 0, 0, 1, 0, 1)), dict(aabb=(0, 0, 0, 1, 1, -1)), dict(aabb=(0, 0, 0, float("nan"), 1, 1)),
       dict(n=-1)]


@pytest.mark.parametrize("over", BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in BAD])
def test_points_input_grad_rejected_before_any_launch(over):
    assert _call(**over) == EINVAL
    if "n" not in over:
        assert _call(**dict(over, n=0)) == 0                     # no points: DREG_OK before anything is examined


def test_points_input_grad_with_no_output_launches_nothing():
    assert _call(grad_x=None, grad_dir=None) == 0               # (made-up addresses: a launch would fault, a memset would fail)


def _ray_call(n=1, n_rays=1, **over):
    from dreg_nerf_amd import lib as L
    a = dict(ray=DEV, t=DEV, grad_x=DEV, grad_dir=DEV, grad_o=DEV, grad_d=DEV)
    a.update(over)
    return L.load().dreg_ngp_samples_ray_grad(n, a["ray"], a["t"], a["grad_x"], a["grad_dir"], n_rays, a["grad_o"], a["grad_d"], None)


RAY_BAD = [dict(n=-1), dict(n_rays=-1), dict(grad_o=None), dict(grad_d=None), dict(ray=None), dict(t=None), dict(grad_x=None), dict(grad_dir=None)]


@pytest.mark.parametrize("over", RAY_BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in RAY_BAD])
def test_samples_ray_grad_rejected_before_any_launch(over):
    assert _ray_call(**over) == EINVAL
    if "n_rays" not in over and "n" not in over:
        assert _ray_call(**dict(over, n_rays=0)) == 0            # no rays: DREG_OK before anything is examined


# --------------------------------------------------------------------------------------------------------------------------- raises, flags, host parts
class _Unbounded:
    unbounded = True


def test_raises():
    from dreg_nerf_amd import field_train, ngp_train, photo_refine as PR
    from dreg_nerf_amd.render import Rays
    o = torch.zeros(2, 3, requires_grad=True)
    d = torch.tensor([[0.0, 0.0, 1.0]] * 2)
    with pytest.raises(ValueError, match='backward="samples"'):                       # the ray backward carries no ray gradient
        ngp_train.render_image_train(object(), None, Rays(o, d), [0, 0, 0, 1, 1, 1], 0.01)
    with pytest.raises(ValueError, match='backward="samples"'):
        ngp_train.render_image_train(object(), None, Rays(d, o), [0, 0, 0, 1, 1, 1], 0.01, backward="rays")
    with pytest.raises(NotImplementedError):
        ngp_train.render_image_train(_Unbounded(), None, Rays(o, d), [0, 0, 0, 1, 1, 1], 0.01, backward="samples")
    with pytest.raises(NotImplementedError):
        field_train.points_input_grad(_Unbounded(), o.detach(), d, None, None)
    with pytest.raises(NotImplementedError):
        field_train.field_points(_Unbounded(), o, d)
    meta = {"aabb_host": [0, 0, 0, 1, 1, 1], "render_step_size": 0.01}
    with pytest.raises(NotImplementedError):
        PR.refine_pose_photometric((_Unbounded(), None, meta), (_Unbounded(), None, meta), torch.eye(4), torch.eye(4)[None], torch.eye(4)[None],
                                   torch.eye(3), 4, 4)
    with pytest.raises(NotImplementedError):
        PR.refine_pose_photometric((object(), None, dict(meta, unbounded=True)), (object(), None, meta), torch.eye(4), torch.eye(4)[None],
                                   torch.eye(4)[None], torch.eye(3), 4, 4)
    with pytest.raises(ValueError):
        PR.refine_pose_photometric((object(), None, {"render_step_size": 0.01}), (object(), None, meta), torch.eye(4), torch.eye(4)[None],
                                   torch.eye(4)[None], torch.eye(3), 4, 4)


def test_flags(monkeypatch):
    from dreg_nerf_amd.config import config_parser
    monkeypatch.setattr(sys, "argv", ["eval_nerf_regtr.py"])
    cfg = config_parser()
    assert cfg.photo_refine is False and cfg.photo_iters == 200 and cfg.photo_rays == 4096 and cfg.photo_lr == 2e-3 and cfg.photo_depth_weight == 0.1
    monkeypatch.setattr(sys, "argv", ["eval_nerf_regtr.py", "--photo_refine", "--photo_iters", "7", "--photo_rays", "128", "--photo_lr", "0.01",
                                      "--photo_depth_weight", "0.5"])
    cfg = config_parser()
    assert cfg.photo_refine and (cfg.photo_iters, cfg.photo_rays, cfg.photo_lr, cfg.photo_depth_weight) == (7, 128, 0.01, 0.5)
    import inspect
    from dreg_nerf_amd import photo_refine as PR
    sig = inspect.signature(PR.refine_pose_photometric).parameters                         # the flags' defaults are the function's
    assert (sig["iters"].default, sig["n_rays"].default, sig["lr"].default, sig["depth_weight"].default) == (200, 4096, 2e-3, 0.1)


def test_photo_refine_scenes_skips_and_writes(tmp_path, capsys):
    """The evaluator's per-scene driver with an injected refinement: a scene without blocks on disk is skipped with a printed line; the file has
    icp.write_refined_metrics' layout with the start errors and the iterations."""
    import importlib
    import json
    EV = importlib.import_module("eval_nerf_regtr")
    a, b = tmp_path / "a.pth", tmp_path / "b.pth"
    a.write_bytes(b"x")
    b.write_bytes(b"x")
    seen = []

    def refine(sp, tp, start, gt):
        seen.append((sp, tp, tuple(start.shape), tuple(gt.shape)))
        return {"R_mean": 0.5, "t_mean": 0.01, "R_med": 0.5, "t_med": 0.01, "time": 1.0, "R_start": 2.0, "t_start": 0.02, "iterations": 5, "skipped": 0}, None
    jobs = [("s1", str(a), str(b), torch.eye(4)[:3].double(), torch.eye(4)[:3].double()), ("s2", str(a), str(tmp_path / "none.pth"), None, None),
            ("s3", "", "", None, None)]
    rows = EV.photo_refine_scenes(None, jobs, None, refine=refine)
    text = capsys.readouterr().out
    assert list(rows) == ["s1"] and seen == [(str(a), str(b), (3, 4), (3, 4))]
    assert "s2: no NeRF blocks on disk, pose not refined photometrically" in text and "s3: no NeRF blocks on disk" in text
    assert "s1: photometric refinement, 5 iterations: R 2.000 -> 0.500 deg" in text
    out = EV.write_photo_refined(str(tmp_path), "test", rows)
    got = json.load(open(tmp_path / "photo_refined_metrics_test.json"))
    assert got == out and got["R_mean"] == 0.5 and got["t_mean"] == 0.01 and got["s1"]["R_start"] == 2.0 and got["s1"]["iterations"] == 5


def test_pose_chain_host_parts():
    """rays_to_block_diff is render.rays_to_block in fp32 and differentiable; sample_camera_rays draws render.pixel_rays' rays; se3_exp is the
    rigid exponential; the loss drops an empty mask."""
    from dreg_nerf_amd import photo_refine as PR, render as R
    gen = torch.Generator().manual_seed(0)
    cams = G.FIX_CAMS
    rays = PR.sample_camera_rays(cams, G.FIX_K, G.FIX_W, G.FIX_H, 500, gen)
    assert rays.origins.shape == (500, 3) and float((rays.viewdirs.norm(dim=1) - 1).abs().max()) < 1e-6
    full = [R.pixel_rays(c, G.FIX_K, G.FIX_W, G.FIX_H) for c in cams]
    pool = torch.cat([f.viewdirs.reshape(-1, 3) for f in full])
    for k in range(0, 500, 50):                                                            # every drawn ray is a pixel ray of its camera
        ci = int((cams[:, :3, 3] - rays.origins[k]).norm(dim=1).argmin())
        assert float((full[ci].viewdirs.reshape(-1, 3) - rays.viewdirs[k]).norm(dim=1).min()) < 1e-6
    assert pool.shape[0] == 4 * G.FIX_W * G.FIX_H
    xi = torch.tensor([0.03, -0.02, 0.05, 0.1, -0.2, 0.3], dtype=torch.float64)
    E = PR.se3_exp(xi)
    assert float((E[:3, :3] @ E[:3, :3].T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-14 and float(torch.linalg.det(E[:3, :3]) - 1) < 1e-14
    assert torch.equal(E[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
    assert abs(PR.pose_errors(E, torch.eye(4))[0] - np.degrees(float(xi[:3].norm()))) < 1e-9
    want = R.rays_to_block(rays, E)
    Gm = E.float().requires_grad_(True)
    got = PR.rays_to_block_diff(rays, Gm)
    assert float((got.origins.detach() - want.origins).abs().max()) < 1e-5 and float((got.viewdirs.detach() - want.viewdirs).abs().max()) < 1e-6
    (got.origins.sum() + got.viewdirs[:, 0].sum()).backward()
    assert Gm.grad is not None and Gm.grad[:3].abs().sum() > 0
    z = torch.zeros(4)
    assert PR.photometric_loss(torch.zeros(4, 3), z, z, torch.zeros(4, 3), z + 1, z, 0.1) == (None, 0)
    loss, k = PR.photometric_loss(torch.ones(4, 3), z + 1, z + 2, torch.zeros(4, 3), torch.tensor([1.0, 1.0, 0.0, 0.6]), z, 0.1)
    assert k == 3 and abs(float(loss) - (0.5 + 0.1 * 1.5)) < 1e-6
