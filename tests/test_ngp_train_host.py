"""NeRF block training on the host: the restated backward of one ray against hand-derived gradients, the occupancy-grid update,
the image loader, the learning-rate milestones and the adaptive ray count.  No GPU needed."""
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

import render_train_restatement as RT  # noqa: E402


def _autograd_ray(sigma, c, dt, g, bkgd=None):
    sigma = sigma.clone().double().requires_grad_(True)
    c = c.clone().double().requires_grad_(True)
    occ = torch.ones(1, sigma.shape[0], dtype=torch.bool)
    tm = torch.arange(sigma.shape[0], dtype=torch.float64)[None]
    rgb, _, _, surv = RT.composite(sigma[None], c[None], occ, tm, dt, bkgd)
    (rgb[0] * torch.as_tensor(g, dtype=torch.float64)).sum().backward()
    return sigma.grad, c.grad, surv[0]


def test_constant_sigma_slab_closed_form():
    # K samples of constant sigma and colour c: C = c (1 - e^{-K s dt}) + b e^{-K s dt}; dC/dsigma_k = dt (T_{k+1} c - S_k) with the sum over k
    # equal to d/ds of C = K dt e^{-K s dt} (c - b)
    K, s, dt = 12, 3.0, 0.0625          # (dt exact in fp32: the restatement rounds it as the kernel does)
    c = torch.tensor([0.2, 0.5, 0.9], dtype=torch.float64)
    b = torch.ones(3, dtype=torch.float64)
    dsig, dc = RT.ray_backward(torch.full((K,), s), c.expand(K, 3), dt, [1.0, 1.0, 1.0], b)
    want = K * dt * math.exp(-K * s * dt) * (c - b).sum()
    assert abs(float(dsig.sum()) - float(want)) < 1e-12
    ga, gca, _ = _autograd_ray(torch.full((K,), s), c.expand(K, 3), dt, [1.0, 1.0, 1.0], b)
    torch.testing.assert_close(dsig, ga, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(dc, gca, rtol=1e-10, atol=1e-12)


def test_two_survivor_ray_hand_derived():
    dt = 0.1
    s = torch.tensor([2.0, 5.0], dtype=torch.float64)
    c = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    g = [0.3, -0.7, 0.2]
    a1, a2 = 1 - math.exp(-0.2), 1 - math.exp(-0.5)
    # C = a1 c1 + (1 - a1) a2 c2 + (1 - a1)(1 - a2) b, b = 0
    dC_ds1 = dt * (1 - a1) * (c[0] - a2 * c[1])
    dC_ds2 = dt * (1 - a1) * (1 - a2) * c[1]
    gt = torch.tensor(g, dtype=torch.float64)
    dsig, dc = RT.ray_backward(s, c, dt, g)
    assert abs(float(dsig[0]) - float((dC_ds1 * gt).sum())) < 1e-12
    assert abs(float(dsig[1]) - float((dC_ds2 * gt).sum())) < 1e-12
    torch.testing.assert_close(dc, torch.stack([a1 * gt, (1 - a1) * a2 * gt]))


def test_early_stopped_samples_get_no_gradient():
    # a dense first sample drives T below 1e-4: the marched samples after it do not survive and get exactly zero gradient
    dt = 0.1
    s = torch.tensor([200.0, 1.0, 1.0, 1.0], dtype=torch.float64)
    c = torch.rand(4, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    gs, gc, surv = _autograd_ray(s, c, dt, [1.0, 1.0, 1.0], torch.ones(3))
    assert surv.tolist() == [True, False, False, False]
    assert torch.all(gs[1:] == 0) and torch.all(gc[1:] == 0)
    dsig, dc = RT.ray_backward(s[:1], c[:1], dt, [1.0, 1.0, 1.0], torch.ones(3))
    torch.testing.assert_close(dsig, gs[:1])
    torch.testing.assert_close(dc, gc[:1])


def test_gradcheck_closed_form_field():
    # sigma(x) = exp(p0 . x + p1), rgb(x) = sigmoid(P x) along one ray: gradcheck of the compositing in float64
    t = torch.linspace(0.05, 1.0, 10, dtype=torch.float64)
    x = torch.stack([t, 0.5 * t, -t], -1)

    def fn(p0, p1, P):
        sigma = torch.exp(x @ p0 + p1)
        rgb = torch.sigmoid(x @ P.T)
        occ = torch.ones(1, 10, dtype=torch.bool)
        out = RT.composite(sigma[None], rgb[None], occ, t[None], 0.1, torch.ones(3, dtype=torch.float64))
        return out[0]

    p0 = torch.tensor([0.5, -0.3, 0.2], dtype=torch.float64, requires_grad=True)
    p1 = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    P = torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1), requires_grad=True)
    assert torch.autograd.gradcheck(fn, (p0, p1, P))


# ------------------------------------------------------------------------------------------------------------ occupancy grid
def _grid(res=8):
    from dreg_nerf_amd import ngp
    g = ngp.OccupancyGrid([-1, -1, -1, 1, 1, 1], res)
    g.train()
    return g


def test_occupancy_warmup_takes_all_cells_and_ema_max():
    g = _grid()
    seen = []

    def fn(x):
        seen.append(x.shape[0])
        assert (x >= -1).all() and (x <= 1).all()
        return torch.where(x[:, 0] > 0, 0.5, 0.001)

    g.every_n_step(0, fn)
    assert seen == [512]
    g.every_n_step(5, fn)                       # not a multiple of 16: no update
    assert seen == [512]
    occ0 = g.occs.clone()
    g.every_n_step(16, lambda x: torch.zeros(x.shape[0]))
    torch.testing.assert_close(g.occs, occ0 * 0.95)          # max(occs * 0.95, 0)
    g.eval()
    with pytest.raises(RuntimeError):
        g.every_n_step(32, fn)


def test_occupancy_binary_uses_min_of_mean_and_threshold():
    g = _grid()
    g._update(0, lambda x: torch.where(x[:, 0] > 0, 1.0, 0.02))   # mean 0.51 > 0.01: threshold 0.01, every cell occupied
    assert bool(g.binary.all())
    g = _grid()
    g._update(0, lambda x: torch.where(x[:, 0] > 0, 0.004, 0.0))  # mean 0.002 < 0.01: threshold 0.002
    assert g.binary.float().mean().item() == 0.5
    assert bool(g.binary[4:].all()) and not bool(g.binary[:4].any())


def test_occupancy_cell_count_after_warmup():
    g = _grid()
    g._update(0, lambda x: torch.where(x[:, 0] > 0.5, 1.0, 0.0))   # 2 of 8 x-slabs occupied: 128 cells
    assert int(g.binary.sum()) == 128
    n = []
    g._update(300, lambda x: (n.append(x.shape[0]), torch.zeros(x.shape[0]))[1])
    assert n == [128 + 128]                       # num_cells // 4 uniform + min(num_cells // 4, occupied) occupied
    g2 = _grid()
    g2._update(0, lambda x: torch.where(x[:, 0] > 0.75, 1.0, 0.0))  # 64 occupied < 128: all of them
    n = []
    g2._update(300, lambda x: (n.append(x.shape[0]), torch.zeros(x.shape[0]))[1])
    assert n == [128 + 64]


# ------------------------------------------------------------------------------------------------------------ images
def _blender_scene(root, n=40, W=16):
    from PIL import Image
    d = os.path.join(root, "obj")
    os.makedirs(d)
    frames = []
    for i in range(n):
        ang = 2 * math.pi * i / n
        c2w = np.eye(4)
        c2w[:3, 3] = [3 * math.cos(ang), 3 * math.sin(ang), 0.5 if i % 2 else -0.5]
        rgba = np.zeros((W, W, 4), np.uint8)
        rgba[..., 0] = 255
        rgba[..., 3] = 0
        rgba[: W // 2, :, 3] = 255               # top half: opaque red; bottom: transparent
        Image.fromarray(rgba, "RGBA").save(os.path.join(d, f"r_{i}.png"))
        frames.append({"file_path": f"r_{i}", "transform_matrix": c2w.tolist()})
    with open(os.path.join(d, "transforms.json"), "w") as fp:
        json.dump({"camera_angle_x": 0.5, "frames": frames}, fp)
    return d


def test_nerf_images_split_compositing_intrinsics(tmp_path):
    from dreg_nerf_amd import nerf_images
    _blender_scene(str(tmp_path))
    tr = nerf_images.SubjectImages.load("objaverse", str(tmp_path), "obj", "train", "cpu")[0]
    te = nerf_images.SubjectImages.load("objaverse", str(tmp_path), "obj", "test", "cpu")[0]
    assert len(tr) == 38 and len(te) == 2                    # frames 0 and 20 are the test split
    torch.testing.assert_close(te.camtoworlds[1, :3, 3], torch.tensor([3 * math.cos(math.pi), 3 * math.sin(math.pi), -0.5]))
    f = 0.5 * 16 / math.tan(0.25)
    torch.testing.assert_close(tr.K, torch.tensor([[f, 0, 8.0], [0, f, 8.0], [0, 0, 1.0]]))
    rays, px = tr.view(0)
    torch.testing.assert_close(px[0, 0], torch.tensor([1.0, 0.0, 0.0]))    # opaque red
    torch.testing.assert_close(px[-1, 0], torch.tensor([1.0, 1.0, 1.0]))   # transparent over white
    torch.testing.assert_close(rays.viewdirs.norm(dim=-1), torch.ones(16, 16))
    with pytest.raises(NotImplementedError):
        nerf_images.load_renderings("scannerf", str(tmp_path), "obj", "train")


def test_nerf_images_kmeans_blocks_stable(tmp_path):
    from dreg_nerf_amd import nerf_images
    _blender_scene(str(tmp_path))
    a = nerf_images.SubjectImages.load("objaverse", str(tmp_path), "obj", "train", "cpu", multi_blocks=True, num_blocks=2)
    b = nerf_images.SubjectImages.load("objaverse", str(tmp_path), "obj", "train", "cpu", multi_blocks=True, num_blocks=2)
    assert len(a) == 2 and [x.current_block for x in a] == [0, 1]
    for x, y in zip(a, b):
        assert torch.equal(x.camtoworlds, y.camtoworlds)
    t = nerf_images.SubjectImages.load("objaverse", str(tmp_path), "obj", "test", "cpu", multi_blocks=True, num_blocks=2)
    assert sum(len(x) for x in a) + sum(len(x) for x in t) == 40


# ------------------------------------------------------------------------------------------------------------ schedule
def test_multistep_lr_milestones_and_num_rays():
    from dreg_nerf_amd import ngp_train
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.Adam([p], lr=1e-2, eps=1e-15)
    sch = ngp_train.multistep_lr(opt, 1000)
    assert sch.milestones == {500: 1, 750: 1, 900: 1} and sch.gamma == 0.33
    lrs = []
    for _ in range(1000):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    assert lrs[499] == 1e-2 and abs(lrs[500] - 3.3e-3) < 1e-12 and abs(lrs[900] - 1e-2 * 0.33 ** 3) < 1e-12
    assert ngp_train.next_num_rays(256, 1 << 16) == 1024
    assert ngp_train.next_num_rays(1000, 3 * (1 << 18)) == 333
    assert abs(ngp_train.render_step_size_of([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]) - 3 * math.sqrt(3) / 1024) < 1e-12
