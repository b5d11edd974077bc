"""CPU restatement of NeRF block training's render rule: the renderer of tests/render_restatement.py with stratified marching
(t_min + u dt per ray) and differentiable in every field parameter, plus the hand-derived backward of one ray that csrc/render_train.hip
implements (dL/dc_k = w_k g, dL/dsigma_k = dt g . (T_{k+1} c_k - S_k)).  Run under autograd it gives reference gradients."""
import contextlib

import numpy as np
import torch

from oracle import ngp_oracle as N


def ray_interval(o, d, scene_aabb):
    """(t_min [R], t_max [R], hit [R]) of the slab test as the kernel forms it (render_ray_interval in csrc/march.h: (face - o) * (1 / d)), so that
    the sample positions, and the hash-grid corners they reach, are the kernel's to the bit."""
    lo, hi = scene_aabb[:3], scene_aabb[3:]
    par = d == 0
    inv = 1.0 / torch.where(par, torch.ones_like(d), d)
    t0, t1 = (lo - o) * inv, (hi - o) * inv
    tlo, thi = torch.minimum(t0, t1), torch.maximum(t0, t1)
    tlo = torch.where(par, torch.full_like(tlo, -1e30), tlo)
    thi = torch.where(par, torch.full_like(thi, 1e30), thi)
    near, far = tlo.max(dim=-1).values, thi.min(dim=-1).values
    hit = (near <= far) & (far > 0) & (~par | ((o >= lo) & (o <= hi))).all(dim=-1)
    return near.clamp(min=0.0), far, hit


def march(o, d, binary, roi_aabb, scene_aabb, dt, jitter=None):
    """(t_mid [R,S], occupied [R,S]) on the lattice t_min + u dt + (n + 1/2) dt (u = jitter [R], 0 when None)."""
    binary = binary.bool().cpu()
    rx, ry, rz = binary.shape
    res = torch.tensor([rx, ry, rz], dtype=torch.float32)
    tmin, tmax, hit = ray_interval(o, d, scene_aabb)
    if jitter is not None:
        tmin = tmin + jitter.float() * np.float32(dt)
    hit = hit & (tmin < tmax)
    span = torch.where(hit, tmax - tmin, torch.zeros_like(tmin))
    S = int(torch.ceil((span / dt).max()).item()) + 1 if o.shape[0] else 1
    n = torch.arange(S, dtype=torch.float32)
    tm = tmin[:, None] + (n[None, :] + 0.5) * np.float32(dt)
    valid = (tm < tmax[:, None]) & hit[:, None]
    x = o[:, None, :] + tm[..., None] * d[:, None, :]
    u = (x - roi_aabb[:3]) / (roi_aabb[3:] - roi_aabb[:3])
    inside = ((u >= 0) & (u <= 1)).all(-1)
    ci = torch.floor(u * res).long()
    ci = torch.minimum(torch.maximum(ci, torch.zeros(3, dtype=torch.long)), torch.tensor([rx - 1, ry - 1, rz - 1]))
    occ = binary[ci[..., 0], ci[..., 1], ci[..., 2]] & inside & valid
    return tm, occ


def composite(sigma, rgb_s, occ, tm, dt, bkgd=None, early_stop_eps=1e-4):
    """nerfacc 0.3.5 rendering of marched samples: sigma [R,S], rgb_s [R,S,3] -> (rgb [R,3], opacity [R], depth [R], survivors [R,S])."""
    R = sigma.shape[0]
    alpha = (1.0 - torch.exp(-sigma * np.float32(dt))) * occ
    with torch.no_grad():
        T_all = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=alpha.dtype), 1.0 - alpha[:, :-1]], dim=1), dim=1)
        surv = occ & (T_all >= early_stop_eps)
    a_s = alpha * surv
    T_s = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=alpha.dtype), 1.0 - a_s[:, :-1]], dim=1), dim=1)
    w = a_s * T_s
    opacity = w.sum(1)
    rgb = (w[..., None] * rgb_s).sum(1)
    if bkgd is not None:
        rgb = rgb + torch.as_tensor(bkgd, dtype=rgb.dtype) * (1.0 - opacity[:, None])
    return rgb, opacity, (w * tm.to(w.dtype)).sum(1), surv


def _f16_ste(t):
    return t + (t.half().float() - t).detach()


@contextlib.contextmanager
def fp32_backward():
    """The oracle's fp16 roundings with fp32 gradients (straight through), the kernel's backward arithmetic: autograd through .half() would
    round every gradient to fp16 (the table gradients of a few hundred rays sit at fp16's subnormal steps of 6e-8)."""
    saved = N.f16
    N.f16 = _f16_ste
    try:
        yield
    finally:
        N.f16 = saved


def render_train(base, color, model_aabb, o, d, binary, roi_aabb, scene_aabb, dt, jitter, bkgd=None, dtype=torch.float32):
    """The training forward over the oracle's NGP network (base = mlp_base.params, color = color_mlp.params, fp32, may require grad):
    (rgb [R,3], opacity [R], depth [R], survivors [R,S]).  sigma = trunc_exp(h0 - 1) whose backward is exp(min(h0 - 1, 15)).  Forward values
    are the oracle's (fp16 roundings); gradients flow in fp32.  dtype = torch.float64: the sums between the fp16 roundings, the compositing and
    the gradients in fp64 (the march and the cell of every sample stay the fp32 ones): the second form of this reference, whose distance from
    the first says what the reference itself can hold (tests/test_render_bwd_host.py, profiles/render_bwd_fp64_ratios.txt)."""
    with fp32_backward():
        return _render_train(base, color, model_aabb, o, d, binary, roi_aabb, scene_aabb, dt, jitter, bkgd, dtype)


def _render_train(base, color, model_aabb, o, d, binary, roi_aabb, scene_aabb, dt, jitter, bkgd, dtype=torch.float32):
    o, d = o.float().cpu(), d.float().cpu()
    roi_aabb, scene_aabb = torch.as_tensor(roi_aabb, dtype=torch.float32), torch.as_tensor(scene_aabb, dtype=torch.float32)
    model_aabb = torch.as_tensor(model_aabb, dtype=torch.float32)
    R = o.shape[0]
    tm, occ = march(o, d, binary, roi_aabb, scene_aabb, dt, jitter)
    S = tm.shape[1]
    idx = torch.nonzero(occ)
    x = o[idx[:, 0]] + tm[idx[:, 0], idx[:, 1], None] * d[idx[:, 0]]
    lo, hi = model_aabb[:3], model_aabb[3:]
    u = (x - lo) / (hi - lo)
    selector = ((u > 0.0) & (u < 1.0)).all(dim=-1)
    w1, w2, table = N.split_density_params(base.to(dtype))
    enc = N.hash_encode(u, N.f16(table)).to(dtype)
    h = N.f16(torch.relu(enc @ N.f16(w1).T))
    raw = N.f16(h @ N.f16(w2).T)
    s = _TruncExp.apply(raw[:, 0] - 1.0) * selector.to(dtype)
    c = N.query_rgb(d[idx[:, 0]], raw, color.to(dtype))
    sigma = torch.zeros(R, S, dtype=dtype).index_put((idx[:, 0], idx[:, 1]), s)
    rgb_s = torch.zeros(R, S, 3, dtype=dtype).index_put((idx[:, 0], idx[:, 1]), c)
    out = composite(sigma, rgb_s, occ, tm, dt, bkgd)
    _LAST_SAMPLES.update(u=u.detach(), ray=idx[:, 0], surv=out[3][idx[:, 0], idx[:, 1]])
    return out


_LAST_SAMPLES = {}     # the marched samples of the last render_train call: u [M,3] in the model aabb, their ray, whether they survived


def reached_entries(rays_mask: torch.Tensor) -> torch.Tensor:
    """bool over the hash table's entries (x 2 features): those a trilinear corner of a surviving sample of the rays in rays_mask reaches with a
    non-zero weight (the last render_train call's samples)."""
    keep = _LAST_SAMPLES["surv"] & rays_mask[_LAST_SAMPLES["ray"]]
    u = _LAST_SAMPLES["u"][keep].clamp(0.0, 1.0)
    ones = torch.ones(N.level_table()[1], 2, requires_grad=True)
    N.hash_encode(u, ones).sum().backward()
    return ones.grad.reshape(-1) != 0


class _TruncExp(torch.autograd.Function):
    """exp with the gradient clamped at exp(15) (the reference's trunc_exp, conerf/radiance_fields/ngp.py:22-38)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15))


def ray_backward(sigma, c, dt, g, bkgd=None):
    """The hand-derived backward of one ray over its survivors (what the kernel applies): sigma [K], c [K,3], g = dL/drgb [3] ->
    (dL/dsigma [K], dL/dc [K,3]).  S_k = C - sum_{j<=k} w_j c_j from the forward colour C."""
    sigma, c, g = sigma.double(), c.double(), torch.as_tensor(g, dtype=torch.float64)
    alpha = 1.0 - torch.exp(-sigma * dt)
    T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1.0 - alpha]), 0)
    w = alpha * T[:-1]
    C = (w[:, None] * c).sum(0)
    if bkgd is not None:
        C = C + torch.as_tensor(bkgd, dtype=torch.float64) * T[-1]
    S = C[None, :] - torch.cumsum(w[:, None] * c, 0)
    dsig = dt * ((T[1:, None] * c - S) * g).sum(-1)
    return dsig, w[:, None] * g[None, :]
