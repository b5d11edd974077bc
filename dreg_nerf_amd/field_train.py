"""Training of a NeRF block's field on POINTS: field_points(field, x, dirs) -> (sigma [N], rgb [N,3]), differentiable with
respect to field.mlp_base.params and field.color_mlp.params.  The forward is the inference forward (dreg_ngp_density_fwd_ws + dreg_ngp_rgb_dir_fwd
on the field's fp16 copies: the bits of query_raw / query_rgb), the backward one dreg_ngp_points_bwd (csrc/field_train.hip).  Positions and
directions receive gradients when they require them: one dreg_ngp_points_input_grad (csrc/field_input_grad.hip); when neither
does, nothing more is launched.  ngp_train.NGPAdam steps the field and refreshes its fp16 copies as for the ray training."""
import torch

from . import lib as L


def points_bwd(field, x, dirs, g_sigma, g_rgb, grad_base=None, grad_color=None):
    """One dreg_ngp_points_bwd launch: the gradients of (g_sigma . sigma + g_rgb . rgb) ADDED into grad_base / grad_color (made as zeros when not
    given).  x, dirs fp32 [N,3] contiguous on the field's device; g_sigma [N] / g_rgb [N,3] or None (zeros).  Returns (grad_base, grad_color)."""
    lib = L.load()
    base16, col16 = field._prepared()
    dev = base16.device
    n = x.shape[0]
    if grad_base is None:
        grad_base = torch.zeros(base16.numel(), dtype=torch.float32, device=dev)
    if grad_color is None:
        grad_color = torch.zeros(col16.numel(), dtype=torch.float32, device=dev)
    if n and (g_sigma is not None or g_rgb is not None):
        nws = int(lib.dreg_ngp_points_bwd_workspace_bytes(n))
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        L.check(lib.dreg_ngp_points_bwd(L.ptr(x), L.ptr(dirs), n, base16.data_ptr(), col16.data_ptr(), *field._levels, L.f6(field._aabb_host()),
                                        L.ptr(g_sigma), L.ptr(g_rgb), L.ptr(grad_base), L.ptr(grad_color), L.ptr(ws), nws, L.stream()),
                "dreg_ngp_points_bwd")
    return grad_base, grad_color


def points_input_grad(field, x, dirs, g_sigma, g_rgb, want_x=True, want_dir=True):
    """One dreg_ngp_points_input_grad launch: (dL/dx [N,3] or None, dL/ddir [N,3] or None) of (g_sigma . sigma + g_rgb . rgb) with the parameters
    frozen; written, not added.  x, dirs fp32 [N,3] contiguous on the field's device; g_sigma [N] / g_rgb [N,3] or None (zeros: the outputs
    are zeros).  dirs is differentiated as given (not renormalised)."""
    if getattr(field, "unbounded", False):
        raise NotImplementedError("points_input_grad: the contracted (unbounded) field is not implemented")
    base16, col16 = field._prepared()
    dev = base16.device
    n = x.shape[0]
    gx = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_x else None
    gd = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_dir else None
    if n and (want_x or want_dir):
        L.check(L.load().dreg_ngp_points_input_grad(L.ptr(x), L.ptr(dirs), n, base16.data_ptr(), col16.data_ptr(), *field._levels,
                                                    L.f6(field._aabb_host()), L.ptr(g_sigma), L.ptr(g_rgb), L.ptr(gx), L.ptr(gd), L.stream()),
                "dreg_ngp_points_input_grad")
    return gx, gd


class _FieldPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, base_params, color_params, field, x, dirs):
        sigma, raw = field.query_raw(x)
        n = x.shape[0]
        rgb = torch.empty(n, 3, dtype=torch.float32, device=x.device)      # query_rgb's launch on raw itself (column 0 is not read)
        L.check(L.load().dreg_ngp_rgb_dir_fwd(L.ptr(raw), *field.color_ptrs(), L.ptr(dirs), L.ptr(rgb), n, L.stream()), "dreg_ngp_rgb_dir_fwd")
        ctx.field = field
        ctx.save_for_backward(x, dirs)
        return sigma, rgb

    @staticmethod
    def backward(ctx, g_sigma, g_rgb):
        x, dirs = ctx.saved_tensors
        gs = None if g_sigma is None else g_sigma.float().contiguous()
        gc = None if g_rgb is None else g_rgb.float().contiguous()
        grad_base = grad_color = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            grad_base, grad_color = points_bwd(ctx.field, x, dirs, gs, gc)
        gx = gd = None
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            gx, gd = points_input_grad(ctx.field, x, dirs, gs, gc, ctx.needs_input_grad[3], ctx.needs_input_grad[4])
        return grad_base, grad_color, None, gx, gd


def field_points(field, x: torch.Tensor, dirs: torch.Tensor):
    """(sigma [N], rgb [N,3]) of the field at the points x [N,3] (its own frame) seen along the directions dirs [N,3] (unit for the field's
    colours; differentiated as given); the bits of field.query_raw(x)[0] and field.query_rgb(dirs, field.query_raw(x)[1][:, 1:]).  x and dirs
    receive gradients when they require them (the straight-through gradient).  Bounded fields only."""
    if getattr(field, "unbounded", False):
        raise NotImplementedError("field_points: the contracted (unbounded) field is not implemented")
    dev = field.mlp_base.params.device
    x = x.reshape(-1, 3).to(dev).float().contiguous()
    dirs = dirs.reshape(-1, 3).to(dev).float().contiguous()
    if x.shape != dirs.shape:
        raise ValueError(f"field_points: {tuple(x.shape)} positions and {tuple(dirs.shape)} directions")
    return _FieldPoints.apply(field.mlp_base.params, field.color_mlp.params, field, x, dirs)
