"""Training of one NeRF block (the reference's train_ngp_nerf.py:268-335, conerf/utils/utils.py:44-141), rule in DESIGN.md §3c:

  render_image_train   the renderer with stratified marching (csrc/render.hip dreg_ngp_render_train) as an autograd Function whose backward is
                       csrc/render_train.hip dreg_ngp_render_bwd: rgb is differentiable w.r.t. mlp_base.params and color_mlp.params;
                       with backward="samples"  the forward keeps its surviving samples as a list (csrc/render_samples.hip) and
                       the backward is dreg_ngp_samples_grad + dreg_ngp_points_bwd: rgb, opacity and depth are all differentiable, also with
                       respect to the rays' origins and viewdirs (dreg_ngp_points_input_grad + dreg_ngp_samples_ray_grad)
  NGPAdam              torch.optim.Adam(lr=1e-2, eps=1e-15) whose step is one fused pass per parameter (dreg_ngp_adam_step) that also refreshes the
                       field's fp16 inference copies and zeroes the gradient; state_dict layout = torch.optim.Adam's
  NGPTrainer           the per-step rule: occupancy update every 16 steps, random rays over the block's images, render, smooth-L1 on the alive
                       rays, Adam, MultiStepLR, and the adaptive ray count that keeps 2^18 rendered samples per step
"""
import math
from typing import Optional

import torch
import torch.nn.functional as F

from . import lib as L
from . import ngp
from . import render as R

TARGET_SAMPLES = 1 << 18
_LAST = {"n": 0}          # surviving samples of the last training forward


def render_step_size_of(aabb) -> float:
    """max(aabb extent) sqrt(3) / 1024 (train_ngp_nerf.py, AABB scenes)."""
    a = [float(v) for v in (aabb.tolist() if torch.is_tensor(aabb) else aabb)]
    return max(a[3] - a[0], a[4] - a[1], a[5] - a[2]) * math.sqrt(3) / 1024


class _RenderTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, base_params, color_params, field, occupancy_grid, o, d, jitter, scene_aabb, dt, bkgd, alpha_thre):
        lib = L.load()
        base16, col16 = field._prepared()
        dev = base16.device
        n = o.shape[0]
        roi, b8, bits = R._grid_parts(occupancy_grid, dev)
        rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
        opacity = torch.empty(n, dtype=torch.float32, device=dev)
        depth = torch.empty(n, dtype=torch.float32, device=dev)
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        L.check(lib.dreg_ngp_render_train(L.ptr(o), L.ptr(d), L.ptr(jitter), n, L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], L.ptr(bits),
                                          *field.density_ptrs(), *field.color_ptrs(),
                                          *field._levels, L.f6(roi), L.f6(scene_aabb), L.f6(field._aabb_host()), -math.inf, math.inf,
                                          float(dt), float(alpha_thre), 1e-4, L.f3(bkgd),
                                          L.ptr(rgb), L.ptr(opacity), L.ptr(depth), counters.data_ptr(), counters.data_ptr() + 8, L.stream()),
                "dreg_ngp_render_train")
        c = counters.cpu()                      # the step's one readback: the surviving samples (next step's ray count)
        if int(c[1]) < 0:
            raise RuntimeError("dreg_ngp_render_train reached its pass bound")
        _LAST["n"] = int(c[0])
        ctx.field, ctx.grid_parts, ctx.scene_aabb, ctx.dt, ctx.alpha_thre = field, (roi, b8, bits), scene_aabb, float(dt), float(alpha_thre)
        ctx.save_for_backward(o, d, jitter, rgb)
        ctx.mark_non_differentiable(opacity, depth)
        return rgb, opacity, depth

    @staticmethod
    def backward(ctx, g_rgb, _g_op, _g_dep):
        lib = L.load()
        o, d, jitter, rgb = ctx.saved_tensors
        field = ctx.field
        base16, col16 = field._prepared()
        dev = base16.device
        roi, b8, bits = ctx.grid_parts
        n = o.shape[0]
        grad_base = torch.zeros(base16.numel(), dtype=torch.float32, device=dev)
        grad_color = torch.zeros(col16.numel(), dtype=torch.float32, device=dev)
        if n and g_rgb is not None:
            nws = int(lib.dreg_ngp_render_bwd_workspace_bytes(n))
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            L.check(lib.dreg_ngp_render_bwd(L.ptr(o), L.ptr(d), L.ptr(jitter), n, L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], L.ptr(bits),
                                            base16.data_ptr(), col16.data_ptr(), *field._levels, L.f6(roi), L.f6(ctx.scene_aabb), L.f6(field._aabb_host()),
                                            -math.inf, math.inf, ctx.dt, ctx.alpha_thre, 1e-4, L.ptr(rgb), L.ptr(g_rgb.float().contiguous()),
                                            L.ptr(grad_base), L.ptr(grad_color), L.ptr(ws), nws, L.stream()), "dreg_ngp_render_bwd")
        return grad_base, grad_color, None, None, None, None, None, None, None, None, None


MAX_DEFAULT_CAPACITY = 1 << 20
BACKWARDS = ("rays", "samples")
_RECORD = (("ray", torch.int32, 1), ("ord", torch.int32, 1), ("t", torch.float32, 1), ("x", torch.float32, 3), ("T_next", torch.float32, 1),
           ("w", torch.float32, 1), ("c", torch.float32, 3), ("P", torch.float32, 3), ("Pd", torch.float32, 1))


def default_sample_capacity(n_rays: int, scene_aabb, dt: float) -> int:
    """min(n_rays * n_max, 2^20), n_max = ceil(scene diagonal / dt) + 2 (march_fill_block's bound on a ray's samples)."""
    a = [float(v) for v in scene_aabb]
    diag = math.sqrt(sum((a[3 + k] - a[k]) ** 2 for k in range(3)))
    return max(1, min(n_rays * (int(math.ceil(diag / dt)) + 2), MAX_DEFAULT_CAPACITY))


def render_train_samples(field, grid_parts, o, d, jitter, scene_aabb, dt, bkgd, alpha_thre, capacity):
    """One dreg_ngp_render_train_samples launch and its one readback: (rgb, opacity, depth, record dict of `capacity` rows, true count)."""
    lib = L.load()
    base16, _ = field._prepared()
    dev = base16.device
    n = o.shape[0]
    roi, b8, bits = grid_parts
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    opacity = torch.empty(n, dtype=torch.float32, device=dev)
    depth = torch.empty(n, dtype=torch.float32, device=dev)
    counters = torch.zeros(3, dtype=torch.int64, device=dev)
    rec = {k: torch.empty((capacity, w) if w > 1 else (capacity,), dtype=dt_, device=dev) for k, dt_, w in _RECORD}
    L.check(lib.dreg_ngp_render_train_samples(L.ptr(o), L.ptr(d), L.ptr(jitter), n, L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], L.ptr(bits),
                                              *field.density_ptrs(), *field.color_ptrs(),
                                              *field._levels, L.f6(roi), L.f6(scene_aabb), L.f6(field._aabb_host()), -math.inf, math.inf,
                                              float(dt), float(alpha_thre), 1e-4, L.f3(bkgd),
                                              L.ptr(rgb), L.ptr(opacity), L.ptr(depth), counters.data_ptr(), counters.data_ptr() + 8,
                                              capacity, *[L.ptr(rec[k]) if capacity else None for k, _, _ in _RECORD],
                                              counters.data_ptr() + 16, L.stream()), "dreg_ngp_render_train_samples")
    c = counters.cpu()                          # the step's one readback: the surviving samples, the overrun flag, the list's true length
    if int(c[1]) < 0:
        raise RuntimeError("dreg_ngp_render_train_samples reached its pass bound")
    assert int(c[0]) == int(c[2])
    return rgb, opacity, depth, rec, int(c[2])


def canonical_order(rec, count):
    """The first `count` records in canonical order, ascending ray then ord: the order the scheduling of the forward cannot change."""
    key = (rec["ray"][:count].to(torch.int64) << 32) | rec["ord"][:count].to(torch.int64)
    perm = torch.argsort(key)
    return {k: v[:count][perm].contiguous() for k, v in rec.items()}


def samples_grad(rec, d, rgb, opacity, depth, g_rgb, g_opacity, g_depth, dt):
    """dreg_ngp_samples_grad on a record dict: (dirs [n,3], g_sigma [n], g_c [n,3]), or None when all three upstream gradients are None."""
    n = rec["ray"].shape[0]
    dev = rec["ray"].device
    if n == 0 or (g_rgb is None and g_opacity is None and g_depth is None):
        return None
    dirs = torch.empty(n, 3, dtype=torch.float32, device=dev)
    g_sigma = torch.empty(n, dtype=torch.float32, device=dev)
    g_c = torch.empty(n, 3, dtype=torch.float32, device=dev)
    L.check(L.load().dreg_ngp_samples_grad(n, *[L.ptr(rec[k]) for k in ("ray", "t", "T_next", "w", "c", "P", "Pd")], L.ptr(d), L.ptr(rgb), L.ptr(opacity),
                                           L.ptr(depth), L.ptr(g_rgb), L.ptr(g_opacity), L.ptr(g_depth), float(dt), L.ptr(dirs), L.ptr(g_sigma),
                                           L.ptr(g_c), L.stream()), "dreg_ngp_samples_grad")
    return dirs, g_sigma, g_c


def samples_ray_grad(field, rec, grads, with_rgb, n_rays):
    """(dL/dorigins [n_rays,3], dL/dviewdirs [n_rays,3]) from samples_grad's output `grads` (None: zeros) on the canonical-order list `rec`:
    dreg_ngp_points_input_grad at rec["x"], then dreg_ngp_samples_ray_grad.  The t_k, the survivor set and the jitter are constants."""
    from . import field_train
    dev = rec["ray"].device
    n = rec["ray"].shape[0]
    grad_o = torch.empty(n_rays, 3, dtype=torch.float32, device=dev)
    grad_d = torch.empty(n_rays, 3, dtype=torch.float32, device=dev)
    if grads is None or n == 0:
        return grad_o.zero_(), grad_d.zero_()
    dirs, g_sigma, g_c = grads
    gx, gdir = field_train.points_input_grad(field, rec["x"], dirs, g_sigma, g_c if with_rgb else None)
    L.check(L.load().dreg_ngp_samples_ray_grad(n, L.ptr(rec["ray"]), L.ptr(rec["t"]), L.ptr(gx), L.ptr(gdir), n_rays, L.ptr(grad_o), L.ptr(grad_d),
                                               L.stream()), "dreg_ngp_samples_ray_grad")
    return grad_o, grad_d


class _RenderTrainSamples(torch.autograd.Function):
    """The training forward that keeps its survivors: rgb, opacity and depth are differentiable; the backward is
    dreg_ngp_samples_grad on the sorted list, then dreg_ngp_points_bwd (parameters that require grad) and dreg_ngp_points_input_grad +
    dreg_ngp_samples_ray_grad (origins / viewdirs that require grad)."""

    @staticmethod
    def forward(ctx, base_params, color_params, field, occupancy_grid, o, d, jitter, scene_aabb, dt, bkgd, alpha_thre, capacity):
        base16, _ = field._prepared()
        parts = R._grid_parts(occupancy_grid, base16.device)
        n = o.shape[0]
        cap = default_sample_capacity(n, scene_aabb, dt) if capacity is None else int(capacity)
        rgb, opacity, depth, rec, count = render_train_samples(field, parts, o, d, jitter, scene_aabb, dt, bkgd, alpha_thre, cap)
        if count > cap:                         # the list did not fit: once more, at its true length (same jitter, fresh counters)
            rgb, opacity, depth, rec, count = render_train_samples(field, parts, o, d, jitter, scene_aabb, dt, bkgd, alpha_thre, count)
        _LAST["n"] = count
        ctx.field, ctx.dt = field, float(dt)
        ctx.set_materialize_grads(False)        # an output the loss does not use arrives as None, and its term is not computed
        ctx.rec = canonical_order(rec, count)
        ctx.save_for_backward(d, rgb, opacity, depth)
        return rgb, opacity, depth

    @staticmethod
    def backward(ctx, g_rgb, g_op, g_dep):
        from . import field_train
        d, rgb, opacity, depth = ctx.saved_tensors
        field = ctx.field
        base16, col16 = field._prepared()
        dev = base16.device
        want_params = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        want_rays = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        grad_base = grad_color = grad_o = grad_d = None
        if want_params:                         # (frozen parameters, field.requires_grad_(False): neither the buffers nor dreg_ngp_points_bwd)
            grad_base = torch.zeros(base16.numel(), dtype=torch.float32, device=dev)
            grad_color = torch.zeros(col16.numel(), dtype=torch.float32, device=dev)
        gs = [None if g is None else g.float().contiguous() for g in (g_rgb, g_op, g_dep)]
        out = samples_grad(ctx.rec, d, rgb, opacity, depth, gs[0], gs[1], gs[2], ctx.dt)
        if out is not None and want_params:
            dirs, g_sigma, g_c = out
            field_train.points_bwd(field, ctx.rec["x"], dirs, g_sigma, g_c if gs[0] is not None else None, grad_base, grad_color)
        if want_rays:                           # through the field into x_k = o + t_k d and dirs_k = d, then along the rays
            grad_o, grad_d = samples_ray_grad(field, ctx.rec, out, gs[0] is not None, d.shape[0])
        return grad_base, grad_color, None, None, grad_o, grad_d, None, None, None, None, None, None


def render_image_train(field, occupancy_grid, rays, scene_aabb, render_step_size: float, render_bkgd=None, alpha_thre: float = 0.0,
                       jitter: Optional[torch.Tensor] = None, backward: str = "rays", sample_capacity: Optional[int] = None):
    """render_image for training (stratified marching, differentiable rgb): rays with origins / viewdirs [N,3] -> (rgb [N,3], opacity [N,1],
    depth [N,1], n_rendering_samples int).  jitter fp32 [N] in [0,1) (the per-ray offset u of t_min + u dt) is drawn with torch.rand when not
    given.  backward="rays": opacity and depth are detached.  backward="samples" (DESIGN.md §3o): the forward keeps its surviving samples
    (sample_capacity records at first, default min(N n_max, 2^20); launched once more at the true count when they do not fit) and all three
    outputs are differentiable, also with respect to rays.origins / rays.viewdirs when they require grad (the sample distances,
    the survivor set and the jitter are constants); the ray backward carries no such gradient and raises."""
    if backward not in BACKWARDS:
        raise ValueError(f"render_image_train: backward must be one of {BACKWARDS}, not {backward!r}")
    if backward != "samples" and torch.is_grad_enabled() and (getattr(rays.origins, "requires_grad", False) or getattr(rays.viewdirs, "requires_grad", False)):
        raise ValueError('render_image_train: origins / viewdirs that require grad need backward="samples" (the ray backward carries no ray gradient)')
    if sample_capacity is not None and int(sample_capacity) < 0:
        raise ValueError("render_image_train: sample_capacity must be >= 0")
    if getattr(field, "unbounded", False) or scene_aabb is None:
        raise NotImplementedError("render_image_train: unbounded scenes are not supported")
    if getattr(getattr(occupancy_grid, "contraction_type", None), "name", "AABB") != "AABB":
        raise NotImplementedError("render_image_train: only ContractionType.AABB occupancy grids")
    base16, _ = field._prepared()
    dev = base16.device
    o = rays.origins.reshape(-1, 3).to(dev).float().contiguous()
    d = rays.viewdirs.reshape(-1, 3).to(dev).float().contiguous()
    n = o.shape[0]
    if jitter is None:
        jitter = torch.rand(n, dtype=torch.float32, device=dev)
    jitter = jitter.to(dev).float().contiguous()
    bk = [0.0, 0.0, 0.0] if render_bkgd is None else [float(v) for v in torch.as_tensor(render_bkgd).reshape(-1).tolist()]
    if backward == "samples":
        rgb, opacity, depth = _RenderTrainSamples.apply(field.mlp_base.params, field.color_mlp.params, field, occupancy_grid, o, d, jitter,
                                                        [float(v) for v in (scene_aabb.tolist() if torch.is_tensor(scene_aabb) else scene_aabb)],
                                                        float(render_step_size), bk, float(alpha_thre or 0.0), sample_capacity)
        return rgb, opacity[:, None], depth[:, None], _LAST["n"]
    rgb, opacity, depth = _RenderTrain.apply(field.mlp_base.params, field.color_mlp.params, field, occupancy_grid, o, d, jitter,
                                             [float(v) for v in (scene_aabb.tolist() if torch.is_tensor(scene_aabb) else scene_aabb)],
                                             float(render_step_size), bk, float(alpha_thre or 0.0))
    return rgb, opacity[:, None], depth[:, None], _LAST["n"]


class NGPAdam(torch.optim.Adam):
    """torch.optim.Adam(field.parameters(), lr, betas, eps) with a fused step: one pass per parameter updates p, exp_avg and exp_avg_sq, writes the
    field's fp16 inference copy (the buffers its renderer reads) and zeroes p.grad.  Same state_dict as torch.optim.Adam."""

    def __init__(self, field: ngp.NGPradianceField, lr: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-15):
        super().__init__([field.mlp_base.params, field.color_mlp.params], lr=lr, betas=betas, eps=eps, foreach=False)
        self.field = field

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        lib = L.load()
        base16, col16 = self.field._prepared()
        copies = {id(self.field.mlp_base.params): base16, id(self.field.color_mlp.params): col16}
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                g = p.grad
                assert g.is_contiguous() and g.dtype == torch.float32
                L.check(lib.dreg_ngp_adam_step(L.ptr(p.data), L.ptr(g), L.ptr(st["exp_avg"]), L.ptr(st["exp_avg_sq"]), copies[id(p)].data_ptr(),
                                               p.numel(), float(group["lr"]), float(b1), float(b2), float(group["eps"]), int(st["step"].item()),
                                               L.stream()), "dreg_ngp_adam_step")
        return None


def multistep_lr(optimizer, max_iterations: int):
    """MultiStepLR(milestones=[max_it // 2, max_it * 3 // 4, max_it * 9 // 10], gamma=0.33) of train_ngp_nerf.py."""
    return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[max_iterations // 2, max_iterations * 3 // 4, max_iterations * 9 // 10],
                                                gamma=0.33)


def next_num_rays(num_rays: int, n_samples: int, target: int = TARGET_SAMPLES) -> int:
    """The ray count of the next step: int(num_rays * target / n_rendering_samples)."""
    return int(num_rays * (target / float(n_samples)))


class NGPTrainer:
    """The per-step rule of train_ngp_nerf.py for one AABB block."""

    def __init__(self, field: ngp.NGPradianceField, grid: ngp.OccupancyGrid, data, aabb, max_iterations: int,
                 target_sample_batch_size: int = TARGET_SAMPLES, backward: str = "rays", opacity_loss_weight: float = 0.0):
        if backward not in BACKWARDS:
            raise ValueError(f"NGPTrainer: backward must be one of {BACKWARDS}, not {backward!r}")
        if not float(opacity_loss_weight) >= 0.0:
            raise ValueError("NGPTrainer: opacity_loss_weight must be >= 0")
        if float(opacity_loss_weight) > 0.0 and backward != "samples":
            raise ValueError('NGPTrainer: opacity_loss_weight > 0 needs backward="samples" (the ray backward carries no opacity gradient)')
        self.backward, self.opacity_loss_weight = backward, float(opacity_loss_weight)
        self.field, self.grid, self.data = field, grid, data
        self.aabb = [float(v) for v in (aabb.tolist() if torch.is_tensor(aabb) else aabb)]
        self.render_step_size = render_step_size_of(self.aabb)
        self.alpha_thre = 0.0
        self.target = int(target_sample_batch_size)
        self.num_rays = self.target // 1024
        self.optimizer = NGPAdam(field, lr=1e-2, eps=1e-15)
        self.scheduler = multistep_lr(self.optimizer, max_iterations)
        self.bkgd = torch.ones(3, dtype=torch.float32)
        self.last = {}

    def occ_eval_fn(self, x):
        return self.field.query_density(x) * self.render_step_size

    def step(self, it: int):
        """One training iteration; returns the loss (float) or None when no sample survived (the step is skipped)."""
        self.field.train()
        self.grid.train()
        self.grid.every_n_step(step=it, occ_eval_fn=self.occ_eval_fn, occ_thre=1e-2)
        alpha = None
        if self.opacity_loss_weight > 0.0:
            rays, pixels, alpha = self.data.sample(self.num_rays, with_alpha=True)
        else:
            rays, pixels = self.data.sample(self.num_rays)
        if self.backward == "samples":
            rgb, opacity, _depth, n = render_image_train(self.field, self.grid, rays, self.aabb, self.render_step_size, self.bkgd, self.alpha_thre,
                                                         backward="samples")
        else:
            rgb, opacity, _depth, n = render_image_train(self.field, self.grid, rays, self.aabb, self.render_step_size, self.bkgd, self.alpha_thre)
        if n == 0:
            return None
        self.num_rays = max(1, next_num_rays(len(pixels), n, self.target))
        alive = opacity.squeeze(-1) > 0
        loss = F.smooth_l1_loss(rgb[alive], pixels[alive])
        if alpha is not None:                    # the mask loss, over ALL rays of the batch (the weight is untuned)
            loss = loss + self.opacity_loss_weight * torch.mean((opacity.squeeze(-1) - alpha) ** 2)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        self.scheduler.step()
        self.last = {"loss": float(loss.detach()), "n_samples": n, "num_rays": len(pixels), "alive": int(alive.sum())}
        return self.last["loss"]
