"""GPU: the fused K-block renderer (csrc/render_scene.hip, dreg_nerf_amd.render.render_scene_image; rule: DESIGN.md §3j), on the generated 32^3
blocks, cameras and option sets of tests/test_hip_render_pair.py.

* K = 1 IS render_image and K = 2 IS render_pair_image, bit for bit; with all grids empty but one / but two, K = 3 and 4 are too.
* K = 3 and 4 overlapping, against the CPU restatement (tests/render_scene_restatement.py), held to the bounds the pair test takes from
  tests/test_hip_render.py: >= 99 % of the pixels within 2e-2 in rgb, opacity and each weight_block column and within 2e-2 relative in depth,
  the surviving-sample count within 1 %.  The poses are chosen on the restatement so that in every case at least 20 % of the survivors are
  covered by two or more OTHER blocks: the general overlap weight is what is tested.
* weight_block sums to the opacity, bit-identity between runs and launch widths, the guards, and register_scene's plumbing end to end."""
import ctypes
import json
import math

import pytest
import torch

import render_scene_restatement as RS
import test_hip_render_pair as TP
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import ngp
from dreg_nerf_amd import render as R

pytestmark = pytest.mark.gpu
DEV, AABB, W, H, K, DT = TP.DEV, TP.AABB, TP.W, TP.H, TP.K, TP.DT
CAMERAS, OPTS = TP.CAMERAS, TP.OPTS
SHELLS = ((3, (0.55, 1.05)), (5, (0.45, 0.95)), (7, (0.5, 1.0)), (9, (0.6, 1.1)))          # (seed, shell) of the four blocks
CENTERS = (TP.C_SRC, TP.C_TGT, torch.tensor([-1.8, 1.5, 0.7]), torch.tensor([0.5, 0.4, 2.3]))  # camera centroids, each in its block's frame


def _rot(axis, deg, t):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    Rm = {"z": [[c, -s, 0], [s, c, 0], [0, 0, 1]], "x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]]}[axis]
    P = torch.eye(4)
    P[:3, :3] = torch.tensor(Rm)
    P[:3, 3] = torch.tensor(t)
    return P


# Block frame -> the rays' frame: 25 / -20 / 15 degrees about z / x / y, and a pure translation for the fourth block.  Up to three blocks, the
# last block of a scene takes the rays as they are (pose None).  The translations (|t| <= 0.24) are chosen on the CPU restatement so that every
# camera first meets a region that at least three shells cover.  Rays go opaque within a few samples, so this is a matter of where the shells'
# near surfaces lie: seen from the two cameras outside, those of the first three shells (outer radii 1.05, 0.95, 1.0) are all at 0.95-0.97, and the
# fourth, largest shell (0.6, 1.1) is moved away from those cameras until its near surface lies below them, but not so far that the camera
# inside comes to stand in its wall.  (Left in place, its outer 0.05 hid the other three: 0.2-0.5 % of the survivors had two or more other
# covering blocks.)  With these poses the restatement counts 26-98 % at K = 4 and 32-87 % at K = 3; asserted per case (>= 20 %).
POSES = (TP.POSE, _rot("x", -20.0, (-0.03, 0.018, 0.094)), _rot("y", 15.0, (-0.072, 0.011, 0.06)), _rot("z", 0.0, (-0.222, 0.013, 0.087)))


def _poses(n):
    return list(POSES) if n == 4 else list(POSES[:n - 1]) + [None]


@pytest.fixture(scope="module")
def four():
    return [TP._block(seed, shell=shell) for seed, shell in SHELLS]


def _empty():
    return ngp.OccupancyGrid(AABB, 32)


def _opts(**kw):
    return dict(scene_aabb=AABB, render_step_size=DT, **kw)


def _scene(blocks, grids, poses, rays, bkgd=None, power=4.0, **opts):
    return R.render_scene_image([(b[0], g, _opts(**opts), CENTERS[i % 4], p) for i, (b, g, p) in enumerate(zip(blocks, grids, poses))], rays,
                                power=power, render_bkgd=bkgd)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------- K = 1 and K = 2: the existing kernels
@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("opts", sorted(OPTS))
def test_one_block_is_render_image_bit_for_bit(four, cam, opts):
    rays = R.pixel_rays(CAMERAS[cam].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    want = R.render_image(four[0][0], four[0][1], rays, AABB, render_step_size=DT, render_bkgd=bk, **OPTS[opts])
    got = _scene(four[:1], [four[0][1]], [None], rays, bkgd=bk, **OPTS[opts])
    assert want[3] > 0 and got[4] == want[3] and _same(got[:3], want[:3])
    assert got[3].shape == (H, W, 1) and torch.equal(got[3], got[1])
    # through a pose: the block's render of the rays brought into its frame
    want = R.render_image(four[0][0], four[0][1], R.rays_to_block(rays, TP.POSE), AABB, render_step_size=DT, render_bkgd=bk, **OPTS[opts])
    got = _scene(four[:1], [four[0][1]], [TP.POSE], rays, bkgd=bk, **OPTS[opts])
    assert got[4] == want[3] and _same(got[:3], want[:3])


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("opts", sorted(OPTS))
def test_two_blocks_are_render_pair_image_bit_for_bit(four, cam, opts):
    src, tgt = four[0], four[1]
    rays = R.pixel_rays(CAMERAS[cam].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    want = TP._render_pair(src, src[1], tgt, tgt[1], rays, bkgd=bk, **OPTS[opts])
    got = _scene([src, tgt], [src[1], tgt[1]], [TP.POSE, None], rays, bkgd=bk, **OPTS[opts])
    assert want[4] > 1000 and got[4] == want[4] and _same(got[:3], want[:3])
    assert got[3].shape == (H, W, 2) and torch.equal(got[3][..., :1], want[3])
    assert 0 < float(got[3][..., 0].sum()) < float(got[1].sum())                 # both blocks contribute
    if opts == "plain":                                                        # another exponent of the overlap weight
        assert _same(_scene([src, tgt], [src[1], tgt[1]], [TP.POSE, None], rays, bkgd=bk, power=1.5)[:3],
                     TP._render_pair(src, src[1], tgt, tgt[1], rays, bkgd=bk, power=1.5)[:3])


# ------------------------------------------------------------------------------------------------------- K = 3, 4 with empty grids
@pytest.mark.parametrize("n", [3, 4])
def test_all_grids_empty_but_one_is_that_blocks_render_bit_for_bit(four, n):
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    poses = _poses(n)
    for i in range(n):
        grids = [four[j][1] if j == i else _empty() for j in range(n)]
        got = _scene(four[:n], grids, poses, rays, bkgd=bk, alpha_thre=1e-2)
        rays_i = rays if poses[i] is None else R.rays_to_block(rays, poses[i])
        want = R.render_image(four[i][0], four[i][1], rays_i, AABB, render_step_size=DT, render_bkgd=bk, alpha_thre=1e-2)
        assert want[3] > 0 and got[4] == want[3] and _same(got[:3], want[:3]), i
        assert torch.equal(got[3][..., i:i + 1], got[1]) and not got[3][..., [j for j in range(n) if j != i]].any(), i


@pytest.mark.parametrize("n,i,j", [(3, 0, 1), (3, 0, 2), (3, 1, 2), (4, 0, 3), (4, 1, 2), (4, 2, 3)])
def test_all_grids_empty_but_two_is_the_pairs_render_bit_for_bit(four, n, i, j):
    """The pair kernel takes the target's rays as they are, so its frame is block j's: the scene's rays are brought there first."""
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    poses = _poses(n)
    grids = [four[b][1] if b in (i, j) else _empty() for b in range(n)]
    got = _scene(four[:n], grids, poses, rays, bkgd=bk)
    rays_i = rays if poses[i] is None else R.rays_to_block(rays, poses[i])
    rays_j = rays if poses[j] is None else R.rays_to_block(rays, poses[j])
    # the same two ray sets through the pair's entry point: block i as the source, block j as the target
    lib = L.load()
    keep = []
    a_i = R._pair_block_args(four[i][0], four[i][1], rays_i, _opts(), CENTERS[i], DEV, keep)
    a_j = R._pair_block_args(four[j][0], four[j][1], rays_j, _opts(), CENTERS[j], DEV, keep)
    nr = H * W
    rgb = torch.empty(nr, 3, device=DEV)
    opac, dep, wsrc = (torch.empty(nr, device=DEV) for _ in range(3))
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)
    L.check(lib.dreg_ngp_render_pair(nr, *a_i, *a_j, 4.0, 1e-4, L.f3([1.0, 1.0, 1.0]), L.ptr(rgb), L.ptr(opac), L.ptr(dep), L.ptr(wsrc),
                                     counters.data_ptr(), counters.data_ptr() + 8, L.stream()), "dreg_ngp_render_pair")
    assert int(counters[0]) > 1000 and got[4] == int(counters[0]) and int(counters[1]) >= 0
    assert torch.equal(got[0].view(-1, 3), rgb) and torch.equal(got[1].view(-1), opac) and torch.equal(got[2].view(-1), dep)
    assert torch.equal(got[3][..., i].reshape(-1), wsrc) and 0 < float(wsrc.sum()) < float(opac.sum())
    others = [b for b in range(n) if b not in (i, j)]
    assert not got[3][..., others].any()


@pytest.mark.parametrize("n", [1, 3, 4])
def test_all_grids_empty_render_the_background(four, n):
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    bk = torch.tensor([0.25, 0.5, 1.0])
    rgb, opac, depth, wb, ns = _scene(four[:n], [_empty() for _ in range(n)], _poses(n), rays, bkgd=bk)
    assert ns == 0 and torch.equal(rgb.cpu(), bk.expand(H, W, 3)) and not opac.any() and not depth.any() and not wb.any() and wb.shape == (H, W, n)


# ------------------------------------------------------------------------------------------------------- K = 3, 4 overlapping vs the restatement
def _restate(four, n, rays, kw, bkgd):
    poses = _poses(n)
    flat = lambda r: (r.origins.reshape(-1, 3).cpu(), r.viewdirs.reshape(-1, 3).cpu())
    blocks = [dict(field=("ngp", b[2], b[3], torch.tensor(AABB)), binary=b[1].binary, roi_aabb=AABB, scene_aabb=AABB, dt=DT, center=CENTERS[i], **kw)
              for i, b in enumerate(four[:n])]
    return RS.render_scene(blocks, [flat(rays if p is None else R.rays_to_block(rays, p)) for p in poses], bkgd=bkgd)


def _compare(hip, ref, n, frac=0.99, tol=2e-2):
    """_compare of tests/test_hip_render_pair.py, with every weight_block column held like opacity."""
    rgb, opac, depth, wb, ns = hip
    rgb, opac, depth, wb = rgb.reshape(-1, 3).cpu(), opac.reshape(-1).cpu(), depth.reshape(-1).cpu(), wb.reshape(-1, n).cpu()
    ok_rgb = ((rgb - ref["rgb"]).abs().max(dim=1).values <= tol).float().mean().item()
    ok_op = ((opac - ref["opacity"]).abs() <= tol).float().mean().item()
    ok_wb = [((wb[:, b] - ref["weight_block"][:, b]).abs() <= tol).float().mean().item() for b in range(n)]
    ok_dep = ((depth - ref["depth"]).abs() <= tol * (ref["depth"].abs() + 0.05)).float().mean().item()
    print(f"within tol: rgb {ok_rgb:.4f} opacity {ok_op:.4f} weight_block {[round(v, 4) for v in ok_wb]} depth {ok_dep:.4f}; survivors {ns} vs {ref['n_samples']}")
    assert ok_rgb >= frac and ok_op >= frac and min(ok_wb) >= frac and ok_dep >= frac, (ok_rgb, ok_op, ok_wb, ok_dep)
    assert abs(ns - ref["n_samples"]) <= max(0.01 * ref["n_samples"], 2), (ns, ref["n_samples"])


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("opts", sorted(OPTS))
def test_overlapping_blocks_match_the_restatement(four, n, cam, opts):
    rays = R.pixel_rays(CAMERAS[cam].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    ref = _restate(four, n, rays, OPTS[opts], bk)
    general = int((ref["surv"] & (ref["n_cover"] >= 2)).sum())
    print(f"K = {n} {cam}/{opts}: {ref['n_samples']} survivors, {general} of them with two or more other covering blocks")
    assert ref["n_samples"] > 1000, "the view sees too little of the scene to test anything"
    assert general >= 0.2 * ref["n_samples"], "too few samples lie where three blocks cover the ray: the general overlap weight is not tested"
    hip = _scene(four[:n], [b[1] for b in four[:n]], _poses(n), rays, bkgd=bk, **OPTS[opts])
    _compare(hip, ref, n)
    share = hip[3].reshape(-1, n).sum(0)
    assert (share > 0).all()                                                  # every block contributes


# ------------------------------------------------------------------------------------------------------- weight_block, determinism
@pytest.mark.parametrize("n", [2, 3, 4])
def test_weight_block_sums_to_the_opacity(four, n):
    """The same positive terms w summed in two orders (per block, then over the blocks; and all in stream order): each partial sum is at most
    the opacity <= 1, every addition rounds by at most 2^-25 of its result, and there are at most S = sum_b n_max_b additions on either side."""
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    _, opac, _, wb, ns = _scene(four[:n], [b[1] for b in four[:n]], _poses(n), rays, bkgd=torch.ones(3))
    S = n * (math.ceil(math.sqrt(27.0) / DT) + 2)
    err = (wb.double().sum(-1, keepdim=True) - opac.double()).abs().max().item()
    print(f"K = {n}: max |sum_b weight_block - opacity| = {err:.3e}, bound {S * 2.0 ** -24:.3e}")
    assert ns > 1000 and err <= S * 2.0 ** -24


def test_bit_identical_between_runs_and_launch_widths(four):
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    run = lambda: _scene(four, [b[1] for b in four], _poses(4), rays, bkgd=torch.ones(3))
    a, b = run(), run()
    assert a[4] > 1000 and a[4] == b[4] and _same(a[:4], b[:4])
    for waves in (1, 7):
        with L.probe() as pr:
            pr.set("dreg_render_scene_set_waves", waves, 0)
            c = run()
        assert c[4] == a[4] and _same(a[:4], c[:4]), waves


# ------------------------------------------------------------------------------------------------------- guards
def test_guards_and_shapes(four):
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    grids = [b[1] for b in four]
    rgb, op, dep, wb, ns = _scene(four[:3], grids[:3], _poses(3), rays)
    assert rgb.shape == (H, W, 3) and op.shape == dep.shape == (H, W, 1) and wb.shape == (H, W, 3) and isinstance(ns, int) and ns > 0
    flat = R.Rays(rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3))
    rgb2, _, _, wb2, ns2 = _scene(four[:3], grids[:3], [p if p is None else p[:3] for p in _poses(3)], flat)      # [N,3] rays, [3,4] poses
    assert rgb2.shape == (H * W, 3) and wb2.shape == (H * W, 3) and ns2 == ns and torch.equal(rgb2.view(H, W, 3), rgb)
    with pytest.raises(ValueError):
        R.render_scene_image([], flat)
    with pytest.raises(ValueError):
        _scene(four + four[:1], grids + grids[:1], _poses(5)[:4] + [None], flat)
    contracted = R.BlockGrid(AABB, four[1][1].binary.to(DEV).to(torch.uint8), contraction_type=ngp.ContractionType.UN_BOUNDED_SPHERE)
    with pytest.raises(NotImplementedError):
        _scene(four[:3], [grids[0], contracted, grids[2]], _poses(3), flat)
    with pytest.raises(NotImplementedError):
        _scene(four[:3], grids[:3], _poses(3), flat, cone_angle=0.004)
    with pytest.raises(NotImplementedError):
        R.render_scene_image([(four[0][0], grids[0], dict(render_step_size=DT), CENTERS[0], None)], flat)        # no scene aabb: unbounded
    four[2][0].train()
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            _scene(four[:3], grids[:3], _poses(3), flat)
    finally:
        four[2][0].eval()
    cpu_block = ngp.NGPradianceField(AABB).eval()                              # a field left on the host
    with pytest.raises(ValueError, match="same device"):
        R.render_scene_image([(four[0][0], grids[0], _opts(), CENTERS[0], None), (cpu_block, grids[1], _opts(), CENTERS[1], None)], flat)


def test_entry_point_rejects_bad_arguments(four):
    """dreg_ngp_render_scene itself: a block count out of range or a null pointer in a block returns DREG_EINVAL with nothing launched (the
    outputs keep their fill), which the Python side turns into an error."""
    lib = L.load()
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    keep = []
    arr = (L.SceneBlock * 2)()
    names = [n for n, _ in L.SceneBlock._fields_]
    for i in range(2):
        args = R._pair_block_args(four[i][0], four[i][1], rays, _opts(), CENTERS[i], DEV, keep)
        for name, v in zip(names, args):
            setattr(arr[i], name, ctypes.cast(v, ctypes.c_void_p) if isinstance(v, ctypes.Array) else v)
    n = H * W
    rgb = torch.full((n, 3), -7.0, device=DEV)
    opac, dep = torch.full((n,), -7.0, device=DEV), torch.full((n,), -7.0, device=DEV)
    wb = torch.full((n, 2), -7.0, device=DEV)
    counters = torch.zeros(2, dtype=torch.int64, device=DEV)

    def call(nb, blocks=arr):
        return lib.dreg_ngp_render_scene(n, nb, ctypes.cast(blocks, ctypes.c_void_p), 4.0, 1e-4, L.f3([0.0, 0.0, 0.0]), L.ptr(rgb), L.ptr(opac),
                                         L.ptr(dep), L.ptr(wb), counters.data_ptr(), counters.data_ptr() + 8, L.stream())
    assert call(0) != 0 and call(5) != 0 and call(-1) != 0
    assert lib.dreg_ngp_render_scene(n, 2, None, 4.0, 1e-4, L.f3([0.0, 0.0, 0.0]), L.ptr(rgb), L.ptr(opac), L.ptr(dep), L.ptr(wb),
                                     counters.data_ptr(), counters.data_ptr() + 8, L.stream()) != 0
    for field in ("origins", "binary", "cw2", "res", "scene_aabb", "center"):
        saved = getattr(arr[1], field)
        setattr(arr[1], field, None)
        rc = call(2)
        setattr(arr[1], field, saved)
        assert rc != 0, field
        with pytest.raises(L.DregError):
            L.check(rc, "dreg_ngp_render_scene")
    torch.cuda.synchronize()
    assert (rgb == -7.0).all() and (opac == -7.0).all() and (wb == -7.0).all() and int(counters[0]) == 0 and int(counters[1]) == 0
    assert call(2) == 0                                                        # and the same array, intact, renders
    torch.cuda.synchronize()
    assert int(counters[0]) > 1000 and (opac >= 0).all()


# ------------------------------------------------------------------------------------------------------- register_scene end to end
def _main(monkeypatch, argv):
    """eval_nerf_regtr.py's main() in this process; it seeds the process, so the random streams are put back."""
    import importlib
    import os
    import random
    import sys

    import numpy as np
    monkeypatch.setattr(sys, "argv", ["eval_nerf_regtr.py"] + argv)
    monkeypatch.syspath_prepend(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
    try:
        importlib.import_module("eval_nerf_regtr").main()
    finally:
        random.setstate(state[0])
        np.random.set_state(state[1])
        torch.set_rng_state(state[2])
        torch.cuda.set_rng_state(state[3], DEV)


def test_evaluator_register_scene_leaves_the_metrics_file_as_it_is(tmp_path, monkeypatch, capsys):
    """eval_nerf_regtr.py --synthetic 2 with and without --register_scene --scene_robust --synthetic_blocks 3 (untrained weights: plumbing).
    metrics_test.json is the same file but for `time`, a host clock around the forward call that differs between ANY two runs."""
    import os

    def without_time(path):
        m = json.load(open(path))
        for row in m.values():
            if isinstance(row, dict) and "time" in row:
                row["time"] = 0.0
        return json.dumps(m, indent=2).encode()
    common = ["--root_dir", str(tmp_path), "--synthetic", "2", "--synthetic_res", "32", "--precision", "fp32"]
    _main(monkeypatch, common + ["--expname", "plain"])
    _main(monkeypatch, common + ["--expname", "scene", "--register_scene", "--scene_robust", "--synthetic_blocks", "3"])
    base = lambda name: os.path.join(str(tmp_path), "eval", name, "synthetic")
    assert without_time(os.path.join(base("scene"), "metrics_test.json")) == without_time(os.path.join(base("plain"), "metrics_test.json"))
    assert sorted(os.listdir(base("plain"))) == ["metrics_test.json"] and sorted(os.listdir(base("scene"))) == ["metrics_test.json", "scene_metrics_test.json"]
    js = json.load(open(os.path.join(base("scene"), "scene_metrics_test.json")))
    assert set(js) == {"shell_0000", "shell_0001", "R_mean", "t_mean", "R_mean_direct", "t_mean_direct"}
    assert all(len(js[s]["blocks"]) == 3 and len(js[s]["edges"]) == 6 for s in ("shell_0000", "shell_0001"))
    assert all(math.isfinite(e[k]) for s in ("shell_0000", "shell_0001") for e in js[s]["edges"] for k in ("residual_rot_deg", "residual_trans", "weight"))
    assert "scene registration, 2 scenes" in capsys.readouterr().out


def _write_checkpoint(path, block, cams):
    """A generated block as the checkpoint train_ngp_nerf.py writes (what load_render_block reads), with its cameras."""
    import os
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"step": 1, "model": {k: v.cpu() for k, v in block[0].state_dict().items()}, "occupancy_grid": block[1].state_dict(), "aabb": AABB,
                "unbounded": False, "near_plane": None, "far_plane": None, "grid_resolution": 32, "contraction_type": ngp.ContractionType.AABB,
                "render_step_size": DT, "alpha_thre": 0.0, "cone_angle": 0.0, "camera_poses": cams, "block_id": 0}, path)


SCENE_CAMS = (torch.stack([CAMERAS["outside"], CAMERAS["partly_missing"]]), CAMERAS["inside"][None], CAMERAS["outside"][None])   # per block, own frame


def test_render_registered_scene_default_path_is_render_scene_image(four, tmp_path, monkeypatch):
    """scene_reg.render_registered_scene with NO injected renderer, on three saved block checkpoints: the blocks are loaded, every block's
    cameras are brought into the anchor frame, and the images written are render_scene_image's of those views, under the ground-truth and the
    'synchronised' poses (here: the ground truth with block 1 moved by 0.05, so that the two sets differ)."""
    import numpy as np
    from PIL import Image

    from dreg_nerf_amd import scene_reg
    monkeypatch.setitem(R.INTRINSICS, "objaverse", (W, H, 60.0, 60.0, 32.0, 24.0))
    T = [torch.eye(4), torch.linalg.inv(POSES[1]), torch.linalg.inv(POSES[2])]            # transform[b]: G_b = T_0 inv(T_b) = POSES[b]
    scene = []
    for b in range(3):
        p = str(tmp_path / f"block_{b}" / "model.pth")
        _write_checkpoint(p, four[b], SCENE_CAMS[b])
        scene.append({"nerf_path": p, "transform": T[b], "block_id": b})
    G_gt = scene_reg.ground_truth(scene)
    assert (G_gt[1].float() - POSES[1]).abs().max().item() <= 1e-6
    G_off = G_gt.clone()
    G_off[1, :3, 3] += 0.05
    out = tmp_path / "scene"
    res = scene_reg.render_registered_scene(str(out), scene, G_gt, G_off, "objaverse", DEV)
    assert len(res["views"]) == 4 and all(v["psnr"] < 60.0 and v["ssim"] < 1.0 for v in res["views"])
    assert json.loads((out / "scene_render_metrics.json").read_text()) == res
    # the same images from render_scene_image directly
    Kc = R.intrinsics("objaverse")[0]
    loaded = [R.load_render_block(b["nerf_path"], DEV) for b in scene]
    u8 = lambda x: (np.clip(x.cpu().numpy(), 0.0, 1.0) * 255).astype(np.uint8)
    views = torch.cat([(G_gt[b] @ SCENE_CAMS[b].double()).float() for b in range(3)])
    for prefix, G in (("gt", G_gt), ("aligned", G_off)):
        d = out / f"{prefix}_scene_images"
        assert len(list(d.iterdir())) == 4 * (2 + 3)
        blocks = [(f, g, R.block_pair_opts(m), SCENE_CAMS[b][:, :3, 3].mean(0), G[b]) for b, (f, g, m) in enumerate(loaded)]
        for i, c2w in enumerate(views):
            rgb, opac, _, wb, ns = R.render_scene_image(blocks, R.pixel_rays(c2w.to(DEV), Kc, W, H), render_bkgd=torch.ones(3))
            assert ns > 0 and np.array_equal(np.asarray(Image.open(d / f"rgb_{i}.png")), u8(rgb)), (prefix, i)
            for b in range(3):
                assert np.array_equal(np.asarray(Image.open(d / f"share_{b}_{i}.png"))[..., 0], u8(wb[..., b])), (prefix, i, b)
    # render_blocks_views is what it called: lists of device tensors, the last view's image equal to the direct call's
    rgbs, depths, shares = R.render_blocks_views(loaded, G_off, views, Kc, W, H)
    assert len(rgbs) == 4 and torch.equal(rgbs[3], rgb) and shares[3].shape == (H, W, 3) and torch.equal(shares[3], wb) and depths[3].shape == (H, W, 1)


def test_evaluator_render_scene_on_a_three_block_tree(four, tmp_path, monkeypatch, capsys):
    """eval_nerf_regtr.py's main() with --render_scene alone (it implies --register_scene) on a hand-made three-block split: the sparse, on-device
    get_scene, the network on every ordered pair, the checkpoints loaded and rendered by the default renderer.  Untrained weights: plumbing."""
    import os

    from dreg_nerf_amd import synth
    monkeypatch.setitem(R.INTRINSICS, "objaverse", (W, H, 60.0, 60.0, 32.0, 24.0))
    root, jd = tmp_path / "data", tmp_path / "json"
    T = {0: torch.eye(4), 1: synth.fixed_pose(), 3: synth.fixed_pose(1)}
    (root / "objaverse" / "images" / "sceneA").mkdir(parents=True)
    jd.mkdir()
    json.dump({str(k): v.tolist() for k, v in T.items()}, open(root / "objaverse" / "images" / "sceneA" / "world_frame_transforms.json", "w"))
    json.dump({"train": [], "test": ["sceneA"]}, open(jd / "objaverse.json", "w"))
    for n, k in enumerate(T):
        d = root / "objaverse" / "nerf_models" / "sceneA" / f"block_{k}"
        _write_checkpoint(str(d / "model.pth"), four[n], SCENE_CAMS[n])
        g, m = synth.shell_grid(32, 20 + k, *synth.shell_radii(32), pose=T[k])
        torch.save(g, d / "voxel_grid.pt")
        torch.save(m, d / "voxel_mask.pt")
    common = ["--root_dir", str(root), "--json_dir", str(jd), "--dataset", "objaverse", "--precision", "fp32"]
    _main(monkeypatch, common + ["--expname", "plain"])
    _main(monkeypatch, common + ["--expname", "scene", "--render_scene"])
    text = capsys.readouterr().out
    assert "sceneA: scene render of 3 blocks" in text and "scene registration, 1 scenes" in text
    base = lambda name: root / "eval" / name / "objaverse"
    strip = lambda p: {k: ({q: v for q, v in r.items() if q != "time"} if isinstance(r, dict) else r) for k, r in json.load(open(p)).items()}
    assert strip(base("scene") / "metrics_test.json") == strip(base("plain") / "metrics_test.json")
    assert sorted(os.listdir(base("plain"))) == ["metrics_test.json"]
    assert sorted(os.listdir(base("scene"))) == ["metrics_test.json", "sceneA", "scene_metrics_test.json"]
    row = json.load(open(base("scene") / "scene_metrics_test.json"))["sceneA"]
    assert [b["block"] for b in row["blocks"]] == [0, 1, 3] and len(row["edges"]) == 6
    d = base("scene") / "sceneA"
    assert sorted(os.listdir(d)) == ["aligned_scene_images", "gt_scene_images", "scene_render_metrics.json"]
    assert len(os.listdir(d / "gt_scene_images")) == len(os.listdir(d / "aligned_scene_images")) == 4 * (2 + 3)
    assert len(json.load(open(d / "scene_render_metrics.json"))["views"]) == 4
    # a block count the synthetic scenes do not have ends the run at once
    with pytest.raises(SystemExit, match="synthetic_blocks"):
        _main(monkeypatch, ["--root_dir", str(tmp_path), "--synthetic", "1", "--synthetic_res", "32", "--register_scene", "--synthetic_blocks", "5", "--expname", "bad"])
    assert not (tmp_path / "eval" / "bad").exists()


def test_register_scene_end_to_end_plumbing(tmp_path):
    """Three synthetic blocks through the UNTRAINED network: six ordered edges, one pose per block, finite residuals, the JSON rows.  This
    is plumbing only — an untrained network's poses mean nothing, and nothing here looks at their values."""
    from dreg_nerf_amd import params, scene_reg, synth
    from dreg_nerf_amd.regtr import NeRFRegTr
    m = NeRFRegTr(precision="fp32")
    m.load_state_dict(params.synth_state_dict(0), strict=True)
    m = m.to(DEV).eval()
    poses = [torch.eye(4), synth.fixed_pose(), torch.linalg.inv(synth.fixed_pose())]
    scene = synth.shell_scene(32, (1, 2, 3), poses)
    assert len(scene) == 3
    out = scene_reg.register_scene(m, scene)
    assert out["G"].shape == (3, 4, 4) and out["G"].dtype == torch.float64 and torch.equal(out["G"][0], torch.eye(4, dtype=torch.float64))
    assert [(e["i"], e["j"]) for e in out["edges"]] == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert all(torch.isfinite(torch.as_tensor(e["pose"])).all() for e in out["edges"])
    assert all(math.isfinite(v) for k in ("residual_rot_deg", "residual_trans", "weights") for v in out["info"][k]) and len(out["info"]["weights"]) == 6
    row = scene_reg.scene_row(out, scene)
    (tmp_path / "scene.json").write_text(json.dumps(row))
    back = json.loads((tmp_path / "scene.json").read_text())
    assert len(back["blocks"]) == 3 and len(back["edges"]) == 6 and back["blocks"][0]["rre"] == 0.0
    assert all(math.isfinite(b[k]) for b in back["blocks"] for k in ("rre", "rte", "rre_direct", "rte_direct"))
