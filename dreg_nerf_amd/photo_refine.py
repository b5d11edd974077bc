"""Photometric refinement of a registration: analysis by synthesis in the iNeRF / nerf2nerf family.  The pose that maps the
source block's frame to the target block's is moved so that the source block, rendered along the target's rays, agrees with the target
block's own render, in colour and in depth; the gradient reaches the pose through the field's input gradients
(csrc/field_input_grad.hip: dreg_ngp_points_input_grad, dreg_ngp_samples_ray_grad) behind ngp_train.render_image_train(backward="samples").

Every default below (lr, depth_weight, iters, n_rays, the 0.5 opacity thresholds, the loss form) was written down, NOT tuned."""
import math

import torch
import torch.nn.functional as F

from . import ngp_train
from . import render as R

OPACITY_THRESHOLD = 0.5          # a ray counts where BOTH renders are more than half opaque (not tuned)
BKGD = (1.0, 1.0, 1.0)


def rays_to_block_diff(rays, G: torch.Tensor):
    """render.rays_to_block in torch-differentiable fp32: rays given in the frame G = [R|t] maps TO, expressed in the frame it maps FROM:
    o' = R^T (o - t), d' = R^T d / |R^T d|.  G: [3,4] or [4,4] on the rays' device; gradients flow into G (and the rays)."""
    Rm, t = G[:3, :3].float(), G[:3, 3].float()
    o = (rays.origins.float() - t) @ Rm                         # row vectors: (R^T v)^T = v^T R
    d = rays.viewdirs.float() @ Rm
    return R.Rays(o, d / torch.linalg.norm(d, dim=-1, keepdim=True))


def se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """Exp of the twist xi = (omega, v) in R^6 as a [4,4] matrix (matrix exponential of [[omega]_x v; 0 0]); differentiable."""
    wx, wy, wz, vx, vy, vz = xi.unbind()
    z = torch.zeros((), dtype=xi.dtype, device=xi.device)
    A = torch.stack([torch.stack([z, -wz, wy, vx]), torch.stack([wz, z, -wx, vy]), torch.stack([-wy, wx, z, vz]), torch.stack([z, z, z, z])])
    return torch.linalg.matrix_exp(A)


def sample_camera_rays(cams: torch.Tensor, K: torch.Tensor, W: int, H: int, n: int, generator: torch.Generator):
    """n rays through uniformly drawn pixel centres of uniformly drawn cameras (cams [N,4,4] camera-to-world, OpenGL): render.pixel_rays'
    origins and unit viewdirs at those pixels, [n,3] each, on cams' device."""
    dev = cams.device
    gdev = generator.device
    ci = torch.randint(0, cams.shape[0], (n,), generator=generator, device=gdev).to(dev)
    x = torch.randint(0, W, (n,), generator=generator, device=gdev).to(dev).float()
    y = torch.randint(0, H, (n,), generator=generator, device=gdev).to(dev).float()
    K = K.to(dev).float()
    cam = torch.stack([(x - K[0, 2] + 0.5) / K[0, 0], -(y - K[1, 2] + 0.5) / K[1, 1], -torch.ones_like(x)], dim=-1)
    c2w = cams.float()[ci]
    d = (cam[:, None, :] * c2w[:, :3, :3]).sum(dim=-1)
    return R.Rays(c2w[:, :3, 3].contiguous(), d / torch.linalg.norm(d, dim=-1, keepdim=True))


def _opts(block):
    field, grid, meta = block
    if getattr(field, "unbounded", False) or bool(meta.get("unbounded", False)):
        raise NotImplementedError("refine_pose_photometric: unbounded blocks are not supported")
    aabb = meta.get("scene_aabb", meta.get("aabb_host"))
    if aabb is None:
        raise ValueError("refine_pose_photometric: a block's meta needs its scene aabb (aabb_host) and render_step_size")
    aabb = [float(v) for v in (aabb.tolist() if torch.is_tensor(aabb) else aabb)]
    return field, grid, aabb, float(meta["render_step_size"]), float(meta.get("alpha_thre") or 0.0)


def _kernel_render(block, rays):
    """The moving block's differentiable render: the sample-list forward without jitter (the inference renderer's samples) and its backward."""
    field, grid, aabb, step, alpha_thre = block
    n = rays.origins.shape[0]
    jitter = torch.zeros(n, dtype=torch.float32, device=rays.origins.device)
    rgb, op, dep, ns = ngp_train.render_image_train(field, grid, rays, aabb, step, torch.tensor(BKGD), alpha_thre, jitter=jitter, backward="samples")
    return rgb, op[:, 0], dep[:, 0], ns


def photometric_loss(C_S, O_S, D_S, C_T, O_T, D_T, depth_weight):
    """mean_m smooth_l1(C_S - C_T) + depth_weight mean_m smooth_l1(D_S - D_T) over m = (O_T > 0.5) & (O_S > 0.5) (O_S detached): (loss, |m|);
    loss is None when m is empty."""
    m = (O_T > OPACITY_THRESHOLD) & (O_S.detach() > OPACITY_THRESHOLD)
    k = int(m.sum())
    if k == 0:
        return None, 0
    return F.smooth_l1_loss(C_S[m], C_T[m]) + depth_weight * F.smooth_l1_loss(D_S[m], D_T[m]), k


class PhotoRefiner:
    """The state of one photometric refinement: the twist xi under Adam, the generator, the two blocks.  step() is one iteration;
    refine_pose_photometric drives it (tools/bench_photo_refine.py times it)."""

    def __init__(self, src, tgt, pose_init, src_cams, tgt_cams, K, W, H, n_rays=4096, lr=2e-3, depth_weight=0.1, symmetric=True, seed=0, moving_render=None):
        self.blocks = (_opts(src), _opts(tgt))
        self.fields = (self.blocks[0][0], self.blocks[1][0])
        self.dev = dev = self.fields[0].mlp_base.params.device
        self.moving_render = _kernel_render if moving_render is None else moving_render
        self.G0 = R._pose44(torch.as_tensor(pose_init)).to(dev).float()
        self.cams = (torch.as_tensor(src_cams).float().to(dev), torch.as_tensor(tgt_cams).float().to(dev))
        self.K, self.W, self.H, self.n_rays = K, int(W), int(H), int(n_rays)
        self.depth_weight, self.symmetric = float(depth_weight), bool(symmetric)
        self.xi = torch.zeros(6, dtype=torch.float32, device=dev, requires_grad=True)
        self.opt = torch.optim.Adam([self.xi], lr=lr)
        self.gen = torch.Generator(device=dev).manual_seed(int(seed))
        self.bk = torch.tensor(BKGD)

    def step(self):
        """One iteration: (loss tensor or None when every mask was empty and nothing moved, mask sizes, rendered samples) per direction."""
        G = se3_exp(self.xi) @ self.G0
        terms, masks, samples = [], [], []
        for moving, fixed, pose in ((0, 1, G),) + (((1, 0, torch.linalg.inv(G)),) if self.symmetric else ()):
            rays = sample_camera_rays(self.cams[fixed], self.K, self.W, self.H, self.n_rays, self.gen)
            ff, fg, fa, fs, ft = self.blocks[fixed]
            with torch.no_grad():
                C_T, O_T, D_T, _ = R.render_image(ff, fg, rays, fa, render_step_size=fs, render_bkgd=self.bk, alpha_thre=ft)
            C_S, O_S, D_S, ns = self.moving_render(self.blocks[moving], rays_to_block_diff(rays, pose))
            C_S, O_S, D_S = C_S.to(self.dev), O_S.to(self.dev), D_S.to(self.dev)
            term, k = photometric_loss(C_S, O_S, D_S, C_T, O_T[:, 0], D_T[:, 0], self.depth_weight)
            masks.append(k)
            samples.append(int(ns))
            if term is not None:
                terms.append(term)
        if not terms:
            return None, masks, samples
        loss = sum(terms)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return loss.detach(), masks, samples

    def pose(self):
        """G = Exp(xi) G0, fp64 [4,4] on the host."""
        return se3_exp(self.xi.detach().double().cpu()) @ self.G0.double().cpu()


def refine_pose_photometric(src, tgt, pose_init, src_cams, tgt_cams, K, W, H, iters=200, n_rays=4096, lr=2e-3, depth_weight=0.1, symmetric=True,
                            seed=0, moving_render=None):
    """Refine pose_init ([3,4] or [4,4], source frame -> target frame) photometrically: (pose fp64 [4,4] on the host, info).

    src, tgt: (field, grid, meta) as render.load_render_block returns them (meta: aabb_host or scene_aabb, render_step_size, alpha_thre);
    src_cams / tgt_cams: the blocks' own cameras [N,4,4] in their own frames; K, W, H: the cameras' intrinsics.
    The pose is G = Exp(xi) G0 with xi in R^6 (rotation vector, translation) on the device under torch.optim.Adam(lr).  Per iteration: n_rays
    pixels are drawn from the target's cameras; the target block is rendered by render_image under no_grad; the source block by
    render_image_train(backward="samples") along rays_to_block_diff(rays, G), jitter 0, parameters frozen; the loss is
        mean_m smooth_l1(C_S - C_T) + depth_weight mean_m smooth_l1(D_S - D_T),   m = (O_T > 0.5) & (O_S.detach() > 0.5);
    with symmetric=True the same with the roles swapped is added: pixels from the source's cameras, the source block rendered under no_grad, the
    target block differentiably along rays_to_block_diff(rays, G^-1).  A term whose mask is empty is dropped; an iteration with no term is skipped.
    lr = 2e-3, depth_weight = 0.1, iters = 200, n_rays = 4096, the 0.5 thresholds and the loss form were written down, NOT tuned.
    info: per iteration the loss (nan when skipped), the mask sizes and the rendered samples of the differentiable renders; "skipped".
    moving_render(block, rays) -> (rgb [n,3], opacity [n], depth [n], samples) replaces the kernel path of the differentiable render (tests)."""
    ref = PhotoRefiner(src, tgt, pose_init, src_cams, tgt_cams, K, W, H, n_rays, lr, depth_weight, symmetric, seed, moving_render)
    frozen = [(p, p.requires_grad) for f in ref.fields for p in (f.mlp_base.params, f.color_mlp.params)]
    info = {"loss": [], "mask": [], "samples": [], "skipped": 0}
    try:
        for p, _ in frozen:                     # frozen parameters: the backward makes no parameter gradient (no dreg_ngp_points_bwd, no buffers)
            p.requires_grad_(False)
        for _ in range(int(iters)):
            loss, masks, samples = ref.step()
            info["mask"].append(masks)
            info["samples"].append(samples)
            info["skipped"] += loss is None
            info["loss"].append(float("nan") if loss is None else loss)
    finally:
        for p, req in frozen:
            p.requires_grad_(req)
    info["loss"] = [float(v) for v in info["loss"]]
    info["iterations"] = int(iters)
    info["xi"] = ref.xi.detach().double().cpu().tolist()
    return ref.pose(), info


def pose_errors(pose, pose_gt):
    """(RRE in degrees, RTE) of a [4,4] / [3,4] pose against the ground truth (the registration metrics' definitions)."""
    P, Q = R._pose44(torch.as_tensor(pose)), R._pose44(torch.as_tensor(pose_gt))
    c = ((P[:3, :3].T @ Q[:3, :3]).trace() - 1.0) / 2.0
    return math.degrees(math.acos(float(c.clamp(-1.0, 1.0)))), float((P[:3, 3] - Q[:3, 3]).norm())


def photo_refine_scene(src_path, tgt_path, pose_start, pose_gt, dataset, device, iters=200, n_rays=4096, lr=2e-3, depth_weight=0.1, seed=0):
    """eval_nerf_regtr.py --photo_refine for one scene: the two blocks from disk, refine_pose_photometric from pose_start ([3,4] / [4,4]), scored
    like the prediction: (row of photo_refined_metrics_{split}.json, pose [4,4]).  The row has ES.summary's keys, the start errors and the
    iterations."""
    import time
    from . import losses as LS
    blocks = [R.load_render_block(p, device) for p in (src_path, tgt_path)]
    K, W, H = R.intrinsics(dataset)
    cams = [b[2]["camera_poses"] for b in blocks]
    torch.cuda.synchronize()
    t0 = time.time()
    pose, info = refine_pose_photometric(blocks[0], blocks[1], pose_start, cams[0], cams[1], K, W, H, iters=iters, n_rays=n_rays, lr=lr,
                                         depth_weight=depth_weight, seed=seed)
    torch.cuda.synchronize()
    dt = time.time() - t0
    gt = torch.as_tensor(pose_gt).reshape(-1, 4)[:3][None].float().cpu()
    start = LS.evaluate_camera_alignment(R._pose44(torch.as_tensor(pose_start))[:3][None].float(), gt)
    err = LS.evaluate_camera_alignment(pose[:3][None].float(), gt)
    row = {"R_mean": float(err["R_error_mean"]), "t_mean": float(err["t_error_mean"]), "R_med": float(err["R_error_med"]), "t_med": float(err["t_error_med"]),
           "time": dt, "R_start": float(start["R_error_mean"]), "t_start": float(start["t_error_mean"]), "iterations": int(info["iterations"]),
           "skipped": int(info["skipped"])}
    return row, pose
