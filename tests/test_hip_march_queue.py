"""GPU: the ray queue's own contract (csrc/march.h march_take, and what each marcher does with a taken ray).  Which lane of which wave takes a
ray, and in which refill round, depends on the ray's place in the input; its result must not.  So rendering a permutation of the rays gives the
permuted outputs bit for bit — for the renderer, the stratified training forward (jitter permuted alike), the two-block renderer and the
persistent visibility labels (points permuted), at 1, 63, 65 and 193 rays that mix hits and misses (less than a wave, a wave and one ray, four
waves with a ragged last one).  And a single wave that is handed 70,000 rays which miss the aabb before 10 that hit uses up a pass's 1024
refill rounds without a live ray, goes round again and still renders the 10.  (The training backward is not here: its slab sums depend on which
rays share a chunk.)  Blocks, cameras and pose are those of tests/test_hip_render_pair.py."""
import pytest
import torch

import test_hip_render_pair as TP
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import ngp_train, visibility
from dreg_nerf_amd import render as R

pytestmark = pytest.mark.gpu
DEV, AABB, DT = TP.DEV, TP.AABB, TP.DT
COUNTS = [1, 63, 65, 193]
BK = torch.tensor([0.25, 0.5, 1.0])


@pytest.fixture(scope="module")
def scene():
    """The two blocks, 193 of the partly-missing camera's rays (every 15th pixel: some miss the aabb, some cross the shell) and a jitter per ray."""
    src, tgt = TP._block(3, shell=(0.55, 1.05)), TP._block(5, shell=(0.45, 0.95))
    rays = R.pixel_rays(TP.CAMERAS["partly_missing"].to(DEV), TP.K, TP.W, TP.H)
    o, d = rays.origins.reshape(-1, 3)[7::15][:193].contiguous(), rays.viewdirs.reshape(-1, 3)[7::15][:193].contiguous()
    assert o.shape[0] == 193
    jitter = torch.rand(193, generator=torch.Generator().manual_seed(9)).to(DEV)
    return src, tgt, o, d, jitter


def _perm(n):
    return torch.randperm(n, generator=torch.Generator().manual_seed(100 + n)).to(DEV)


def _same(got, want, perm, n_out):
    """got: the outputs for the permuted rays; want: for the rays as given.  The last entry of each is the surviving-sample count."""
    assert got[-1] == want[-1]
    for g, w in zip(got[:n_out], want[:n_out]):
        assert torch.equal(g, w[perm])


@pytest.mark.parametrize("n", COUNTS)
def test_render_of_permuted_rays_is_the_permuted_render(scene, n):
    _, (f, occ, _, _), o, d, _ = scene
    p = _perm(n)
    want = R.render_image(f, occ, R.Rays(o[:n], d[:n]), AABB, render_step_size=DT, render_bkgd=BK)
    got = R.render_image(f, occ, R.Rays(o[:n][p], d[:n][p]), AABB, render_step_size=DT, render_bkgd=BK)
    _same(got, want, p, 3)
    if n == 193:
        assert 0 < int((want[1] == 0).sum()) < n and want[3] > 0, "the rays must mix hits and misses"


@pytest.mark.parametrize("n", COUNTS)
def test_train_forward_of_permuted_rays_is_the_permuted_forward(scene, n):
    _, (f, occ, _, _), o, d, jitter = scene
    p = _perm(n)
    with torch.no_grad():
        want = ngp_train.render_image_train(f, occ, R.Rays(o[:n], d[:n]), AABB, DT, BK, jitter=jitter[:n])
        got = ngp_train.render_image_train(f, occ, R.Rays(o[:n][p], d[:n][p]), AABB, DT, BK, jitter=jitter[:n][p])
    _same(got, want, p, 3)
    if n == 193:
        assert 0 < int((want[1] == 0).sum()) < n and want[3] > 0


def _pair(src, tgt, o, d):
    opts = TP._opts()
    return R.render_pair_image(src[0], src[1], tgt[0], tgt[1], R.Rays(o, d), TP.POSE, opts, opts, TP.C_SRC, TP.C_TGT, power=4.0, render_bkgd=BK)


@pytest.mark.parametrize("n", COUNTS)
def test_pair_render_of_permuted_rays_is_the_permuted_render(scene, n):
    src, tgt, o, d, _ = scene
    p = _perm(n)
    want = _pair(src, tgt, o[:n], d[:n])
    got = _pair(src, tgt, o[:n][p], d[:n][p])
    _same(got, want, p, 4)
    if n == 193:
        assert 0 < int((want[1] == 0).sum()) < n and 0 < float(want[3].sum()) < float(want[1].sum()), "hits and misses, samples of both blocks"


@pytest.mark.parametrize("n", COUNTS)
def test_persistent_labels_of_permuted_points_are_the_permuted_labels(scene, n):
    """One camera, so n points are n rays: points inside and outside the shell, seen through it from outside the aabb."""
    _, (f, occ, _, _), _, _, _ = scene
    assert visibility.PERSISTENT and visibility.COARSE
    pts = ((torch.rand(193, 3, generator=torch.Generator().manual_seed(21)) - 0.5) * 2.4).to(DEV)[:n]
    cams = torch.tensor([[2.5, 0.3, 0.1]], device=DEV)
    binary = occ.binary.to(DEV)
    p = _perm(n)
    want = visibility.surface_visibility(pts, cams, f, binary, AABB, AABB, DT).clone()
    got = visibility.surface_visibility(pts[p].contiguous(), cams, f, binary, AABB, AABB, DT)
    visibility.OVERRUN.check(wait=True)
    assert torch.equal(got, want[p])
    if n == 193:
        assert 0 < int(want.sum()) < n, "labelled and unlabelled points"


@pytest.mark.parametrize("form", ["render", "pair"])
def test_one_wave_outlasts_a_pass_of_refill_rounds_without_a_live_ray(scene, form):
    """One wave, 70,000 rays that miss every aabb, then 10 that hit: 1024 rounds x 64 lanes = 65,536 rays are taken and written as background in
    the first pass, no lane is live, the queue is not empty — the wave goes round again (`continue`) and renders the rest."""
    src, tgt, o, d, _ = scene
    hit = (R.render_image(tgt[0], tgt[1], R.Rays(o, d), AABB, render_step_size=DT, render_bkgd=BK)[1].reshape(-1) > 0).nonzero().reshape(-1)[:10]
    assert hit.numel() == 10
    n_miss = 70000
    o_all = torch.cat([torch.tensor([0.0, 0.0, 10.0], device=DEV).expand(n_miss, 3), o[hit]]).contiguous()      # above the blocks, looking up
    d_all = torch.cat([torch.tensor([0.0, 0.0, 1.0], device=DEV).expand(n_miss, 3), d[hit]]).contiguous()
    if form == "render":
        run = lambda oo, dd: R.render_image(tgt[0], tgt[1], R.Rays(oo, dd), AABB, render_step_size=DT, render_bkgd=BK)
        knob, n_out = "dreg_render_set_waves", 3
    else:
        run = lambda oo, dd: _pair(src, tgt, oo, dd)
        knob, n_out = "dreg_render_pair_set_waves", 4
    want = run(o[hit].contiguous(), d[hit].contiguous())
    with L.probe() as pr:
        pr.set(knob, 1, 0)
        got = run(o_all, d_all)
    assert got[-1] == want[-1] > 0
    assert torch.equal(got[0][:n_miss], BK.to(DEV).expand(n_miss, 3))
    for g, w in zip(got[1:n_out], want[1:n_out]):
        assert not g[:n_miss].any() and torch.equal(g[n_miss:], w)
    assert torch.equal(got[0][n_miss:], want[0])
