"""CPU restatement of the volume renderer's rule (csrc/render.hip, DESIGN.md "Volume renderer"): nerfacc 0.3.5 ray_marching(sigma_fn,
early_stop_eps, alpha_thre, stratified=False) + rendering(rgb_sigma_fn, render_bkgd) as the reference's render_image calls them.  nerfacc is
absent from the reference tree, so this states the rule rather than pinning parity.  Built on the oracle's networks (oracle.ngp_oracle) and the
marching of oracle.visibility_oracle (slab test, lattice midpoints, floor + clamp cell lookup over the roi aabb).

The field is either the oracle's NGP network (`field = ("ngp", mlp_base_params, color_params, model_aabb)`) or a closed-form stand-in
(`field = callable(x [M,3], d [M,3]) -> (sigma [M], rgb [M,3])`) for the tests that check the rule itself."""
import numpy as np
import torch

from oracle import ngp_oracle as N


def ray_interval(o, d, scene_aabb, near_plane=None, far_plane=None):
    """(t_min [R], t_max [R], hit [R]) of rays o, d [R,3] against the scene aabb (visibility_oracle's slab rule; a direction component of 0 keeps
    the slab when the origin lies in it), then clamped to the near / far planes."""
    lo, hi = scene_aabb[:3], scene_aabb[3:]
    par = d == 0
    safe = torch.where(par, torch.ones_like(d), d)
    t0, t1 = (lo - o) / safe, (hi - o) / safe
    tlo, thi = torch.minimum(t0, t1), torch.maximum(t0, t1)
    inside_slab = (o >= lo) & (o <= hi)
    tlo = torch.where(par, torch.full_like(tlo, -1e30), tlo)
    thi = torch.where(par, torch.full_like(thi, 1e30), thi)
    near, far = tlo.max(dim=-1).values, thi.min(dim=-1).values
    hit = (near <= far) & (far > 0) & (~par | inside_slab).all(dim=-1)
    tmin, tmax = near.clamp(min=0.0), far
    if near_plane is not None:
        tmin = torch.clamp(tmin, min=float(near_plane))
    if far_plane is not None:
        tmax = torch.clamp(tmax, max=float(far_plane))
    return tmin, tmax, hit & (tmin < tmax)


def march(o, d, binary, roi_aabb, scene_aabb, dt, near_plane=None, far_plane=None):
    """The marched samples of every ray: (t_mid [R,S], occupied [R,S]) on the lattice t_min + (n + 1/2) dt, n < S."""
    binary = binary.bool().cpu()
    rx, ry, rz = binary.shape
    res = torch.tensor([rx, ry, rz], dtype=torch.float32)
    tmin, tmax, hit = ray_interval(o, d, scene_aabb, near_plane, far_plane)
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


def _field_eval(field, x, d):
    if callable(field):
        return field(x, d)
    _, base, color, model_aabb = field
    sigma, raw = N.query_density(x, model_aabb, base)
    return sigma, N.query_rgb(d, raw, color)


def render(field, o, d, binary, roi_aabb, scene_aabb, dt, near_plane=None, far_plane=None, bkgd=None, alpha_thre=0.0, early_stop_eps=1e-4):
    """(rgb [R,3], opacity [R], depth [R], n_samples int, survivors [R,S] bool, alpha [R,S]) of rays o, d [R,3] (CPU fp32)."""
    o, d = o.float().cpu(), d.float().cpu()
    roi_aabb, scene_aabb = torch.as_tensor(roi_aabb, dtype=torch.float32), torch.as_tensor(scene_aabb, dtype=torch.float32)
    R = o.shape[0]
    tm, occ = march(o, d, binary, roi_aabb, scene_aabb, dt, near_plane, far_plane)
    S = tm.shape[1]
    idx = torch.nonzero(occ)
    sigma = torch.zeros(R, S)
    rgb_s = torch.zeros(R, S, 3)
    if idx.shape[0]:
        x = o[idx[:, 0]] + tm[idx[:, 0], idx[:, 1], None] * d[idx[:, 0]]
        s, c = _field_eval(field, x, d[idx[:, 0]])
        sigma[idx[:, 0], idx[:, 1]] = s.float()
        rgb_s[idx[:, 0], idx[:, 1]] = c.float()
    alpha = (1.0 - torch.exp(-sigma * np.float32(dt))) * occ
    # T_all: exclusive product over ALL marched samples (unoccupied lattice points have alpha 0); survivors: T_all >= eps [and alpha >= alpha_thre]
    T_all = torch.cumprod(torch.cat([torch.ones(R, 1), 1.0 - alpha[:, :-1]], dim=1), dim=1)
    surv = occ & (T_all >= early_stop_eps)
    if alpha_thre > 0:
        surv = surv & (alpha >= alpha_thre)
    a_s = alpha * surv
    T_s = torch.cumprod(torch.cat([torch.ones(R, 1), 1.0 - a_s[:, :-1]], dim=1), dim=1)
    w = a_s * T_s
    opacity = w.sum(1)
    rgb = (w[..., None] * rgb_s).sum(1)
    if bkgd is not None:
        rgb = rgb + torch.as_tensor(bkgd, dtype=torch.float32) * (1.0 - opacity[:, None])
    depth = (w * tm).sum(1)
    return rgb, opacity, depth, int(surv.sum()), surv, alpha
