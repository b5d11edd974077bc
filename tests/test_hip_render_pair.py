"""GPU: the fused two-block renderer (csrc/render_pair.hip, dreg_nerf_amd.render.render_pair_image; rule: DESIGN.md §3e).

* One block empty: the pair's result IS the other block's render_image, bit for bit (with omega = 1 a sample's arithmetic is ngp_render_kernel's).
* Overlapping blocks against the CPU restatement (tests/render_pair_restatement.py), held to the bounds tests/test_hip_render.py holds the
  one-block renderer to for the same arithmetic (fp16 networks on both sides, different summation orders and exp implementations): >= 99 % of
  the pixels within 2e-2 in rgb, opacity and weight_src and within 2e-2 relative in depth, the surviving-sample count within 1 %.
* Blocks disjoint in depth: the pair's result is the front block's render composited over the back block's, from the device's own one-block
  renders, to 2e-4 (a front ray that ended at T_all < 1e-4 drops at most 1e-4 of the back; the rest is fp32 accumulation).
* Bit-identity between runs and launch widths; the guards of render_image."""
import math

import pytest
import torch

import render_pair_restatement as RP
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import ngp
from dreg_nerf_amd import render as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
W, H = 64, 48
K = torch.tensor([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1]])
DT = 0.02


def _block(seed=3, res=32, shell=(0.55, 1.05)):
    """The generated block of tests/test_hip_render.py (random hash grid and MLPs, a thick occupancy shell), on the device."""
    g = torch.Generator().manual_seed(seed)
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params[:3072] = torch.randn(3072, generator=g) * 1.0
        f.mlp_base.params[3072:] = torch.randn(f.mlp_base.params.numel() - 3072, generator=g)
        f.color_mlp.params.copy_(torch.randn(7168, generator=g) * 0.2)
    base, color = f.mlp_base.params.detach().clone(), f.color_mlp.params.detach().clone()
    c = (torch.arange(res, dtype=torch.float32) + 0.5) / res * 3 - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    rad = torch.stack([X, Y, Z], -1).norm(dim=-1)
    binary = (rad > shell[0]) & (rad < shell[1])
    occ = ngp.OccupancyGrid(AABB, res)
    occ._binary.copy_(binary)
    return f.to(DEV).eval(), occ, base, color


def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target, up = torch.tensor(eye), torch.tensor(target), torch.tensor(up)
    back = torch.nn.functional.normalize(eye - target, dim=0)          # OpenGL: the camera looks down its -z
    right = torch.nn.functional.normalize(torch.linalg.cross(up, back), dim=0)
    true_up = torch.linalg.cross(back, right)
    c2w = torch.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, true_up, back, eye
    return c2w


CAMERAS = {                                                            # CAMERAS of tests/test_hip_render.py
    "outside": _look_at((2.6, -1.9, 1.2), (0.0, 0.0, 0.0)),
    "inside": _look_at((0.2, 0.1, 0.3), (1.0, 0.5, -0.4)),
    "partly_missing": _look_at((2.8, 2.6, 0.4), (1.2, 1.2, 0.0)),
}
OPTS = {"plain": dict(), "alpha_thre": dict(alpha_thre=1e-2), "near_far": dict(near_plane=0.4, far_plane=3.2)}


def _pose():
    """Source frame -> target frame: 25 degrees about z, then t = (-0.13, 0.02, 0.02).  The translation is chosen on the CPU restatement so that
    every camera first meets the region BOTH shells cover: 50-96 % of the survivors of each of the nine cases below carry omega < 1 and the source
    contributes 36-58 % of the opacity.  (With t = (0.3, -0.2, 0.1) the outside camera met the source's shell alone before the rays went
    opaque: 1.7 % of its survivors had omega < 1.)"""
    a = math.radians(25.0)
    P = torch.eye(4)
    P[:3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    P[:3, 3] = torch.tensor([-0.13, 0.02, 0.02])
    return P


POSE = _pose()
C_SRC, C_TGT = torch.tensor([0.3, -2.2, 0.6]), torch.tensor([2.1, 0.4, 0.5])        # camera centroids, each in its block's frame


@pytest.fixture(scope="module")
def pair():
    return _block(3, shell=(0.55, 1.05)), _block(5, shell=(0.45, 0.95))


def _empty():
    return ngp.OccupancyGrid(AABB, 32)


def _opts(**kw):
    return dict(scene_aabb=AABB, render_step_size=DT, **kw)


def _render_pair(src, src_occ, tgt, tgt_occ, rays, pose=POSE, bkgd=None, power=4.0, **opts):
    return R.render_pair_image(src[0], src_occ, tgt[0], tgt_occ, rays, pose, _opts(**opts), _opts(**opts), C_SRC, C_TGT, power=power, render_bkgd=bkgd)


# ------------------------------------------------------------------------------------------------------- exactness: one block empty
@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("opts", sorted(OPTS))
def test_one_block_empty_is_the_other_blocks_render_bit_for_bit(pair, cam, opts):
    src, tgt = pair
    kw = OPTS[opts]
    rays = R.pixel_rays(CAMERAS[cam].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    # the source's grid all zero: the target block's render of the rays as they are
    want = R.render_image(tgt[0], tgt[1], rays, AABB, render_step_size=DT, render_bkgd=bk, **kw)
    got = _render_pair(src, _empty(), tgt, tgt[1], rays, bkgd=bk, **kw)
    assert want[3] > 0 and got[4] == want[3]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert not got[3].any()
    # the target's grid all zero: the source block's render of the rays brought into its frame
    rays_s = R.rays_to_block(rays, POSE)
    want = R.render_image(src[0], src[1], rays_s, AABB, render_step_size=DT, render_bkgd=bk, **kw)
    got = _render_pair(src, src[1], tgt, _empty(), rays, bkgd=bk, **kw)
    assert want[3] > 0 and got[4] == want[3]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert torch.equal(got[3], got[1])


def test_both_blocks_empty_render_the_background(pair):
    src, tgt = pair
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    bk = torch.tensor([0.25, 0.5, 1.0])
    rgb, opac, depth, wsrc, ns = _render_pair(src, _empty(), tgt, _empty(), rays, bkgd=bk)
    assert ns == 0 and torch.equal(rgb.cpu(), bk.expand(H, W, 3)) and not opac.any() and not depth.any() and not wsrc.any()


# ------------------------------------------------------------------------------------------------------- overlapping blocks vs the restatement
def _restate(pair, rays, kw, bkgd):
    src, tgt = pair
    mk = lambda b, c: dict(field=("ngp", b[2], b[3], torch.tensor(AABB)), binary=b[1].binary, roi_aabb=AABB, scene_aabb=AABB, dt=DT, center=c, **kw)
    flat = lambda r: (r.origins.reshape(-1, 3).cpu(), r.viewdirs.reshape(-1, 3).cpu())
    return RP.render_pair(mk(src, C_SRC), mk(tgt, C_TGT), flat(R.rays_to_block(rays, POSE)), flat(rays), bkgd=bkgd)


def _compare(hip, ref, frac=0.99, tol=2e-2):
    """_compare of tests/test_hip_render.py, with weight_src held like opacity."""
    rgb, opac, depth, wsrc, ns = hip
    rgb, opac, depth, wsrc = rgb.reshape(-1, 3).cpu(), opac.reshape(-1).cpu(), depth.reshape(-1).cpu(), wsrc.reshape(-1).cpu()
    ok_rgb = ((rgb - ref["rgb"]).abs().max(dim=1).values <= tol).float().mean().item()
    ok_op = ((opac - ref["opacity"]).abs() <= tol).float().mean().item()
    ok_ws = ((wsrc - ref["weight_src"]).abs() <= tol).float().mean().item()
    ok_dep = ((depth - ref["depth"]).abs() <= tol * (ref["depth"].abs() + 0.05)).float().mean().item()
    print(f"within tol: rgb {ok_rgb:.4f} opacity {ok_op:.4f} weight_src {ok_ws:.4f} depth {ok_dep:.4f}; survivors {ns} vs {ref['n_samples']}")
    assert ok_rgb >= frac and ok_op >= frac and ok_ws >= frac and ok_dep >= frac, (ok_rgb, ok_op, ok_ws, ok_dep)
    assert abs(ns - ref["n_samples"]) <= max(0.01 * ref["n_samples"], 2), (ns, ref["n_samples"])


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("opts", sorted(OPTS))
def test_overlapping_blocks_match_the_restatement(pair, cam, opts):
    src, tgt = pair
    rays = R.pixel_rays(CAMERAS[cam].to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    ref = _restate(pair, rays, OPTS[opts], bk)
    shared = int((ref["surv"] & (ref["omega"] < 1)).sum())
    print(f"{cam}/{opts}: {ref['n_samples']} survivors, {shared} of them with omega < 1")
    assert ref["n_samples"] > 1000, "the view sees too little of the pair to test anything"
    assert shared >= 0.1 * ref["n_samples"], "too few samples lie where both blocks cover the ray: the overlap weight is not tested"
    hip = _render_pair(src, src[1], tgt, tgt[1], rays, bkgd=bk, **OPTS[opts])
    _compare(hip, ref)
    assert 0 < float(hip[3].sum()) < float(hip[1].sum())                 # both blocks contribute


# ------------------------------------------------------------------------------------------------------- disjoint in depth: front over back
@pytest.mark.parametrize("front_part", ["all", "upper_half"])
def test_blocks_disjoint_in_depth_composite_front_over_back(pair, front_part):
    """The target keeps x > 0.2, the source x < -0.2, identity pose, camera on the +x axis at x = 0.7 looking down -x: every target sample lies
    before every source sample and omega = 1 throughout.  The whole source lies behind the (mostly opaque) target; with the target cut down
    to its upper half as well, the lower half of the image shows the source alone next to pixels that show the target alone.
    Tolerance 2e-4 absolute: the merged stream ends once T_all < 1e-4, so it drops at most 1e-4 of weight that the two separate renders keep
    (in rgb, opacity and weight_src), and in the un-normalised depth at most 1e-4 t_max; from x = 0.7 the source's farthest sample, on its
    outer radius 1.05, lies at t <= 1.75, so the depth bound is 1.75e-4.  (From x = 3 it would be 4e-4.)  The rest is fp32 accumulation."""
    src, tgt = pair
    c = (torch.arange(32, dtype=torch.float32) + 0.5) / 32 * 3 - 1.5                 # cell centres along an axis
    keep_t = (c > 0.2)[:, None, None] & ((c > 0)[None, None, :] if front_part == "upper_half" else torch.ones(1, 1, 32, dtype=torch.bool))
    front, back = ngp.OccupancyGrid(AABB, 32), ngp.OccupancyGrid(AABB, 32)
    front._binary.copy_(tgt[1].binary.cpu() & keep_t)
    back._binary.copy_(src[1].binary.cpu() & (c < -0.2)[:, None, None])
    rays = R.pixel_rays(_look_at((0.7, 0.0, 0.0), (0.0, 0.0, 0.0)).to(DEV), K, W, H)
    bk = torch.tensor([1.0, 1.0, 1.0])
    kw = dict(render_step_size=DT)
    rgb_t0, op_t, dep_t, ns_t = R.render_image(tgt[0], front, rays, AABB, render_bkgd=torch.zeros(3), **kw)
    # (the source marches the rays rays_to_block hands it: under the identity pose the same origins, the directions re-normalised in fp64)
    rgb_s, op_s, dep_s, ns_s = R.render_image(src[0], back, R.rays_to_block(rays, torch.eye(4)), AABB, render_bkgd=bk, **kw)
    assert ns_t > 1000 and ns_s > 1000
    rgb, op, dep, wsrc, ns = _render_pair(src, back, tgt, front, rays, pose=torch.eye(4), bkgd=bk)
    tol = 2e-4
    err = lambda a, b: (a - b).abs().max().item()
    e = (err(rgb, rgb_t0 + (1 - op_t) * rgb_s), err(op, op_t + (1 - op_t) * op_s), err(dep, dep_t + (1 - op_t) * dep_s), err(wsrc, (1 - op_t) * op_s))
    t_only = int(((op_t > 0.5) & ((1 - op_t) * op_s < 1e-3)).sum())
    s_only = int(((op_t == 0) & (op_s > 0.5)).sum())
    print(f"max abs error of rgb, opacity, depth, weight_src: {e}; pixels of the target alone {t_only}, of the source alone {s_only}; survivors {ns} of {ns_t} + {ns_s}")
    assert max(e) <= tol, e
    assert ns <= ns_t + ns_s and t_only > 100 and (s_only > 100 or front_part == "all")


# ------------------------------------------------------------------------------------------------------- determinism, guards
def test_bit_identical_between_runs_and_launch_widths(pair):
    src, tgt = pair
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    run = lambda: _render_pair(src, src[1], tgt, tgt[1], rays, bkgd=torch.ones(3))
    a, b = run(), run()
    assert a[4] == b[4] and all(torch.equal(x, y) for x, y in zip(a[:4], b[:4]))
    for waves in (1, 7):
        with L.probe() as pr:
            pr.set("dreg_render_pair_set_waves", waves, 0)
            c = run()
        assert c[4] == a[4] and all(torch.equal(x, y) for x, y in zip(a[:4], c[:4])), waves


def test_guards_and_shapes(pair):
    src, tgt = pair
    rays = R.pixel_rays(CAMERAS["outside"].to(DEV), K, W, H)
    rgb, op, dep, wsrc, ns = _render_pair(src, src[1], tgt, tgt[1], rays)
    assert rgb.shape == (H, W, 3) and op.shape == dep.shape == wsrc.shape == (H, W, 1) and isinstance(ns, int) and ns > 0
    flat = R.Rays(rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3))
    rgb2, _, _, wsrc2, ns2 = _render_pair(src, src[1], tgt, tgt[1], flat, pose=POSE[:3])          # [N,3] rays, [3,4] pose
    assert rgb2.shape == (H * W, 3) and wsrc2.shape == (H * W, 1) and ns2 == ns and torch.equal(rgb2.view(H, W, 3), rgb)
    contracted = R.BlockGrid(AABB, tgt[1].binary.to(DEV).to(torch.uint8), contraction_type=ngp.ContractionType.UN_BOUNDED_SPHERE)
    with pytest.raises(NotImplementedError):
        _render_pair(src, src[1], tgt, contracted, flat)
    with pytest.raises(NotImplementedError):
        _render_pair(src, src[1], tgt, tgt[1], flat, cone_angle=0.004)
    src[0].train()
    try:
        with pytest.raises(RuntimeError, match="inference only"):
            _render_pair(src, src[1], tgt, tgt[1], flat)
    finally:
        src[0].eval()


# ------------------------------------------------------------------------------------------------------- the device side of --render_merged
def test_pair_views_and_merged_metrics(pair):
    """render_pair_views takes the centroids from the blocks' cameras and renders over white; the metrics between two stacks of merged views are
    PSNR 60 / SSIM 1 exactly for the same pose and lower for a pose that is 0.05 off."""
    src, tgt = pair
    cams_s, cams_t = torch.stack([CAMERAS["outside"], CAMERAS["partly_missing"]]), torch.stack([CAMERAS["inside"], CAMERAS["outside"]])
    meta = lambda cams: dict(aabb_host=AABB, render_step_size=DT, camera_poses=cams)
    blocks = ((src[0], src[1], meta(cams_s)), (tgt[0], tgt[1], meta(cams_t)))
    views = torch.stack([CAMERAS["outside"], CAMERAS["partly_missing"]])
    rgbs, depths, shares = R.render_pair_views(blocks, POSE, views, K, W, H)
    assert len(rgbs) == len(depths) == len(shares) == 2 and rgbs[0].shape == (H, W, 3) and depths[0].shape == shares[0].shape == (H, W, 1)
    direct = R.render_pair_image(src[0], src[1], tgt[0], tgt[1], R.pixel_rays(views[1].to(DEV), K, W, H), POSE, _opts(), _opts(),
                                 cams_s[:, :3, 3].mean(0), cams_t[:, :3, 3].mean(0), render_bkgd=torch.ones(3))
    assert torch.equal(rgbs[1], direct[0]) and torch.equal(depths[1], direct[2]) and torch.equal(shares[1], direct[3])
    psnr, ssim = R._stack_metrics(rgbs, [x.clone() for x in rgbs])
    assert psnr == [60.0, 60.0] and ssim == [1.0, 1.0]
    off = POSE.clone()
    off[:3, 3] += 0.05
    psnr, ssim = R._stack_metrics(R.render_pair_views(blocks, off, views, K, W, H)[0], rgbs)
    print("a pose 0.05 off costs: psnr", psnr, "ssim", ssim)
    assert all(p < 60.0 for p in psnr) and all(s < 1.0 for s in ssim)
