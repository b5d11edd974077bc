"""CPU: the fp64 restatement of the point-wise field backward (tests/field_points_restatement.py) against torch autograd on a general field;
the planted errors against the GPU test's bound; the argument guards of dreg_ngp_points_bwd; and the host parts of the scene distiller
(dreg_nerf_amd/scene_merge.py): the colour blend, the sampler, the loss, the flag."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import field_points_restatement as FP
import render_bwd_cases as B
import render_train_restatement as RT
import test_hip_field_train as G
from oracle import ngp_oracle as N
from render_bwd_restatement import MATRICES


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("which", ["sigma", "rgb", "both"])
def test_restatement_equals_autograd_on_a_general_field(which):
    """backward64, fed the oracle's own forward record of a random non-flat field, against autograd through oracle.ngp_oracle.query_density /
    query_rgb: relative L2 <= 1e-4 per matrix and per table level (§3c's figure for the same comparison).  Autograd differentiates the sigmoid
    at its unrounded value s, the rule at the fp16 colour c: the record's c is s here (the one place the two differ by more than fp32
    rounding; the flat-field test holds the kernel to c)."""
    gen = torch.Generator().manual_seed(3)
    n = 1500
    aabb = torch.tensor([-0.6, -0.55, -0.65, 0.55, 0.6, 0.5])
    x = (torch.rand(n, 3, generator=gen) - 0.5) * 1.6
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    base = torch.empty(3072 + N.n_grid_params()).uniform_(-0.5, 0.5, generator=gen)
    base[:3072].uniform_(-0.3, 0.3, generator=gen)
    color = torch.empty(7168).uniform_(-0.3, 0.3, generator=gen)
    gs = torch.randn(n, generator=gen) * (which != "rgb")
    gc = torch.randn(n, 3, generator=gen) * (which != "sigma")
    base.requires_grad_(True)
    color.requires_grad_(True)
    with RT.fp32_backward():                     # the oracle's fp16 roundings with fp32 gradients: .half() would round every gradient to fp16
        sig, raw = N.query_density(x, aabb, base)
        rgb = N.query_rgb(d, raw, color)
        ((sig * gs).sum() + (rgb * gc).sum()).backward()
    record, weights, inside = FP.forward_record(x, d, base.detach(), color.detach(), aabb)
    assert np.array_equal(record["c"], rgb.detach().double().numpy()) and 100 < int((~inside).sum()) < n - 100
    record["c"] = record["s"]
    res = FP.backward64(record, weights, gs.numpy() if which != "rgb" else None, gc.numpy() if which != "sigma" else None, B.levels(), aabb.tolist())
    assert np.array_equal(res.inside, inside)
    gb, gcol = base.grad.double().numpy(), color.grad.double().numpy()
    ref = G.split(gb, gcol)
    for k in MATRICES:
        if which == "sigma" and k.startswith("c"):
            assert not ref[k].any() and not res.val[k].any()
            continue
        r = _rel(res.val[k], ref[k])
        print(f"restatement vs autograd ({which}), {k}: rel L2 {r:.3e}")
        assert r <= 1e-4, (k, r)
    assert not gcol[6144 + 192:].any()
    tab = gb[3072:]
    dense = np.zeros_like(tab)
    dense[res.t_idx] = res.t_val
    for l, row in enumerate(N.level_table()[0]):
        s = slice(2 * row["offset"], 2 * (row["offset"] + row["size"]))
        r = _rel(dense[s], tab[s])
        print(f"restatement vs autograd ({which}), table level {l}: rel L2 {r:.3e} over {int((tab[s] != 0).sum())} elements")
        assert r <= 1e-4, (l, r)


def test_flat_cases_are_what_the_gpu_test_needs():
    """Gradient only at the lane and chunk edges; hits inside and outside the model aabb; every level of the table and all five matrices reached."""
    for n in G.EDGE_COUNTS + (G.WIDE,):
        c = G.flat_case(n)
        assert set(np.nonzero(c.g_sigma)[0]) == set(c.hits) == set(np.nonzero(c.g_rgb.any(1))[0])
        assert set(c.hits) == {p for p in G.HIT_LANES + (n - 1,) if p < n}
        lo, hi = np.array(G.MODEL[:3], np.float32), np.array(G.MODEL[3:], np.float32)
        inside = ((c.x > lo) & (c.x < hi)).all(1)
        assert inside[c.hits[0]] and (n == 1 or (~inside[c.hits]).any()) and (n < 63 or (~inside).sum() > 10)
        assert np.abs(np.linalg.norm(c.d, axis=1) - 1).max() < 1e-6
        res = G.flat_reference(c, B.levels())
        assert set(np.unique(res.t_level)) == set(range(16)) and all(np.abs(res.val[k]).sum() > 0 for k in MATRICES)
        assert np.array_equal(res.inside, inside[c.hits])


@pytest.mark.parametrize("mutate", FP.MUTATIONS)
def test_every_mutation_is_seen(mutate):
    """Each planted error moves an element of the flat case beyond four times the bound the GPU test holds the kernel to."""
    c = G.flat_case(129)
    lv = B.levels()
    res, bad = G.flat_reference(c, lv), G.flat_reference(c, lv, mutate=mutate)
    bnd = G.bounds(res, B.H0[G.DENS])
    worst = 0.0
    for k in MATRICES:
        m = bnd[k] > 0
        if m.any():
            worst = max(worst, float((np.abs(bad.val[k] - res.val[k])[m] / bnd[k][m]).max()))
    dense, dbad = {}, {}
    for i, v in zip(res.t_idx, res.t_val):
        dense[int(i)] = v
    for i, v in zip(bad.t_idx, bad.t_val):
        dbad[int(i)] = v
    tb = dict(zip((int(i) for i in res.t_idx), bnd["table"]))
    for i in set(dense) | set(dbad):
        diff = abs(dense.get(i, 0.0) - dbad.get(i, 0.0))
        worst = max(worst, diff / tb[i] if i in tb else (np.inf if diff > 0 else 0.0))
    print(f"{mutate}: {worst:.3g} x the bound")
    assert worst > 4.0


# --------------------------------------------------------------------------------------------------------------------------- the entry's guards
EINVAL = -1
DEV = 0x10000                 # stands for a device buffer: the entry point reads through none of them on the host
_u16 = (ctypes.c_uint32 * 16)(*range(16))
_f16 = (ctypes.c_float * 16)(*[1.0] * 16)
LEVELS = [ctypes.addressof(_u16)] * 3 + [ctypes.addressof(_f16), ctypes.addressof(_u16)]


def _call(n=1, ws_short=0, aabb=(0, 0, 0, 1, 1, 1), **over):
    from dreg_nerf_amd import lib as L
    lib = L.load()
    box = (ctypes.c_float * 6)(*aabb) if aabb is not None else None           # (kept alive until the call returns)
    a = dict(x=DEV, dirs=DEV, base16=DEV, color16=DEV, offset=LEVELS[0], size=LEVELS[1], res=LEVELS[2], scale=LEVELS[3], hashed=LEVELS[4],
             aabb=ctypes.addressof(box) if box is not None else None, g_sigma=DEV, g_rgb=DEV, grad_base=DEV, grad_color=DEV, ws=DEV)
    a.update(over)
    nws = int(lib.dreg_ngp_points_bwd_workspace_bytes(max(n, 1))) - ws_short
    return lib.dreg_ngp_points_bwd(a["x"], a["dirs"], n, a["base16"], a["color16"], a["offset"], a["size"], a["res"], a["scale"], a["hashed"], a["aabb"],
                                   a["g_sigma"], a["g_rgb"], a["grad_base"], a["grad_color"], a["ws"], nws, None)


BAD = [dict(x=None), dict(dirs=None), dict(base16=None), dict(color16=None), dict(offset=None), dict(size=None), dict(res=None), dict(scale=None),
       dict(hashed=None), dict(aabb=None), dict(grad_base=None), dict(grad_color=None), dict(ws=None), dict(ws_short=1),
       dict(aabb=(0, 0, 0, 1, 0, 1)), dict(aabb=(0, 0, 0, 1, 1, -1)), dict(aabb=(0, 0, 0, float("nan"), 1, 1)), dict(n=-1)]


@pytest.mark.parametrize("over", BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in BAD])
def test_rejected_before_any_launch(over):
    assert _call(**over) == EINVAL
    if "n" not in over:
        assert _call(**dict(over, n=0)) == 0                     # no points: DREG_OK before anything is examined


def test_workspace_rule():
    from dreg_nerf_amd import lib as L
    lib = L.load()
    ws = lambda n: int(lib.dreg_ngp_points_bwd_workspace_bytes(n))
    assert ws(0) == 0 and ws(-3) == 0
    assert ws(1) == ws(64) == 10240 * 4 + 256 and ws(65) == 2 * 10240 * 4 + 256
    assert ws(131072) == 2048 * 10240 * 4 + 256 and ws(131073) == 1025 * 10240 * 4 + 256      # 128-point chunks from 131,073 points on


# --------------------------------------------------------------------------------------------------------------------------- the distiller's host parts
def test_blend_known_answers():
    from dreg_nerf_amd.scene_merge import blend_colors
    t = lambda *v: torch.tensor(v, dtype=torch.float32)
    c0, c1 = torch.tensor([[0.25, 0.5, 0.75]] * 5), torch.tensor([[0.5, 0.125, 1.0]] * 5)
    inf = float("inf")
    #            one carrier (1), one carrier (0), none, a tie, an infinite a
    a0, a1 = t(0.0, 0.3, 0.0, 2.0, inf), t(0.7, 0.0, 0.0, 2.0, 1.0)
    out = blend_colors([a0, a1], [c0, c1])
    assert torch.equal(out[0], c1[0]) and torch.equal(out[1], c0[1])              # bit for bit, not (a c) / a
    assert not out[2].any()
    assert torch.equal(out[3], (2.0 * c0[3] + 2.0 * c1[3]) / 4.0)                 # a tie blends: (a c0 + a c1) / 2a
    assert torch.equal(out[4], c0[4])                                             # not finite: the colour of the largest a
    out = blend_colors([t(inf, inf), t(inf, 1.0), t(0.0, inf)], [c0[:2], c1[:2], torch.tensor([[0.0, 1.0, 0.0]] * 2)])
    assert torch.equal(out[0], c0[0])                                             # a tie of the largest: the lowest index
    assert torch.equal(out[1], c0[1])                                             # inf == inf: block 0 before block 2
    out = blend_colors([t(0.0, 0.5), t(0.0, 0.0)], [None, None])                  # a block whose colour was not queried counts as 0
    assert not out[0].any()


def test_dirs_to_frame_is_the_transpose():
    from dreg_nerf_amd.scene_merge import dirs_to_frame
    from dreg_nerf_amd.synth import fixed_pose
    R = fixed_pose(0)[:3, :3].numpy().astype(np.float32)
    d = torch.nn.functional.normalize(torch.randn(50, 3, generator=torch.Generator().manual_seed(1)), dim=-1)
    torch.testing.assert_close(dirs_to_frame(R, d), d @ torch.from_numpy(R), rtol=1e-6, atol=1e-6)


def test_sampler_stays_inside_and_falls_back_to_uniform():
    from dreg_nerf_amd.scene_merge import sample_points
    aabb = [-1.0, 0.5, 2.0, 3.0, 1.0, 2.5]
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])
    res = (8, 4, 16)
    keep = torch.tensor([0, 5, 8 * 4 * 16 - 1, 100])
    x, d = sample_points(aabb, keep, res, 1001, torch.Generator().manual_seed(0), "cpu")
    assert x.shape == (1001, 3) and d.shape == (1001, 3)
    assert bool(((x >= lo) & (x <= hi)).all()) and float((d.norm(dim=1) - 1).abs().max()) < 1e-5
    u = (x[:500] - lo) / (hi - lo) * torch.tensor(res)
    cell = u.floor().clamp(max=torch.tensor(res) - 1).long()
    flat = (cell[:, 0] * 4 + cell[:, 1]) * 16 + cell[:, 2]
    near = ((u - u.round()).abs() < 1e-4).any(dim=1)                               # on a cell face within rounding: either neighbour
    assert set(flat[~near].tolist()) <= set(keep.tolist()) and len(set(flat.tolist())) >= 4
    x2, _ = sample_points(aabb, keep, res, 1001, torch.Generator().manual_seed(0), "cpu")
    assert torch.equal(x, x2)                                                      # one generator: the same draws
    xe, _ = sample_points(aabb, torch.zeros(0, dtype=torch.long), res, 1000, torch.Generator().manual_seed(0), "cpu")
    ue = (xe - lo) / (hi - lo)
    assert bool(((ue >= 0) & (ue <= 1)).all()) and float(ue.mean()) == pytest.approx(0.5, abs=0.03) and float(ue.std()) == pytest.approx(12 ** -0.5, abs=0.02)


def test_loss_three_point_case():
    from dreg_nerf_amd.scene_merge import distill_loss
    e = np.e
    ss, st = torch.tensor([e - 1, 0.0, e * e - 1]), torch.tensor([0.0, 0.0, e - 1])          # log1p: (1, 0, 2) against (0, 0, 1)
    cs = torch.tensor([[0.5, 0.5, 0.5], [0.1, 0.2, 0.3], [0.5, 0.25, 3.0]])
    ct = torch.tensor([[0.0, 0.0, 0.0], [0.9, 0.9, 0.9], [0.0, 0.25, 1.0]])
    # density term (1 + 0 + 1) / 3; colour term over point 2 alone: smooth_l1 of (0.5, 0, 2) = (0.125, 0, 1.5) -> mean 1.625 / 3
    assert float(distill_loss(ss, cs, st, ct)) == pytest.approx(2.0 / 3.0 + 1.625 / 3.0, rel=1e-6)
    assert float(distill_loss(ss, cs, torch.zeros(3), ct)) == pytest.approx((1.0 + 0.0 + 4.0) / 3.0, rel=1e-6)   # no carrier: no colour term


def test_merge_scene_flag_parses_and_implies_register_scene():
    import eval_nerf_regtr as E
    from dreg_nerf_amd.config import config_parser
    cfg = config_parser([])
    assert cfg.merge_scene is False and cfg.merge_iterations == 2000 and cfg.merge_points == 65536 and E.implied_flags(cfg).register_scene is False
    cfg = E.implied_flags(config_parser(["--merge_scene", "--merge_iterations", "150", "--merge_points", "8192"]))
    assert cfg.merge_scene is True and cfg.register_scene is True and cfg.merge_iterations == 150 and cfg.merge_points == 8192
    assert cfg.scene_voxel_grid is False and cfg.render_scene is False
