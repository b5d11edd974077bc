"""CPU restatement of the two-block renderer's rule (csrc/render_pair.hip), built on tests/render_restatement.py: each block is
marched on its own lattice exactly as the one-block rule marches it, the two sample streams are merged by t_mid (the source's sample first on a
tie), a sample that the other block covers as well is weighted by inverse distance to the blocks' camera centroids, and the merged stream is
composited by the one-block rule (T_all over all samples, survivors, weights over the survivors, early stop).

A block is a dict: field (as render_restatement takes it: ("ngp", base, color, model_aabb) or a callable), binary, roi_aabb, scene_aabb, dt,
center, and optionally near_plane, far_plane, alpha_thre.  Rays are given per block, each in its own frame (dreg_nerf_amd.render.rays_to_block)."""
import numpy as np
import torch

import render_restatement as RR


def covered(block, o, d, t):
    """Whether `block` covers the parameter t [R,S] of its rays o, d [R,3]: t inside [t_min, t_max) of the ray, o + t d inside the roi in an
    occupied cell (floor + clamp, as RR.march looks cells up)."""
    roi = torch.as_tensor(block["roi_aabb"], dtype=torch.float32)
    scene = torch.as_tensor(block["scene_aabb"], dtype=torch.float32)
    binary = block["binary"].bool().cpu()
    rx, ry, rz = binary.shape
    tmin, tmax, hit = RR.ray_interval(o, d, scene, block.get("near_plane"), block.get("far_plane"))
    inside_t = hit[:, None] & (t >= tmin[:, None]) & (t < tmax[:, None])
    x = o[:, None, :] + t[..., None] * d[:, None, :]
    u = (x - roi[:3]) / (roi[3:] - roi[:3])
    inside = ((u >= 0) & (u <= 1)).all(-1)
    ci = torch.floor(u * torch.tensor([rx, ry, rz], dtype=torch.float32)).long()
    ci = torch.minimum(torch.maximum(ci, torch.zeros(3, dtype=torch.long)), torch.tensor([rx - 1, ry - 1, rz - 1]))
    return binary[ci[..., 0], ci[..., 1], ci[..., 2]] & inside & inside_t, x


def render_pair(src, tgt, rays_src, rays_tgt, power=4.0, bkgd=None, early_stop_eps=1e-4, use_omega=True):
    """Rays (o, d) [R,3] per block -> dict(rgb [R,3], opacity [R], depth [R], weight_src [R], n_samples int, and per merged sample [R,S_S+S_T],
    in composited order: is_src, t, omega, alpha, surv).  use_omega=False leaves the overlap weight out (what double counting would give)."""
    blocks = (src, tgt)
    rays = [(o.float().cpu(), d.float().cpu()) for o, d in (rays_src, rays_tgt)]
    R = rays[0][0].shape[0]
    tm, occ, sigma, rgb_s, xs = [], [], [], [], []
    for b, (o, d) in zip(blocks, rays):
        t_b, occ_b = RR.march(o, d, b["binary"], torch.as_tensor(b["roi_aabb"], dtype=torch.float32),
                              torch.as_tensor(b["scene_aabb"], dtype=torch.float32), b["dt"], b.get("near_plane"), b.get("far_plane"))
        S = t_b.shape[1]
        idx = torch.nonzero(occ_b)
        s_b, c_b = torch.zeros(R, S), torch.zeros(R, S, 3)
        if idx.shape[0]:
            x = o[idx[:, 0]] + t_b[idx[:, 0], idx[:, 1], None] * d[idx[:, 0]]
            s, c = RR._field_eval(b["field"], x, d[idx[:, 0]])
            s_b[idx[:, 0], idx[:, 1]] = s.float()
            c_b[idx[:, 0], idx[:, 1]] = c.float()
        tm.append(t_b); occ.append(occ_b); sigma.append(s_b); rgb_s.append(c_b)
    # overlap weight of every sample: the other block's coverage at the same ray parameter
    omega = []
    for i in (0, 1):
        j = 1 - i
        cov, x_other = covered(blocks[j], rays[j][0], rays[j][1], tm[i])
        x_own = rays[i][0][:, None, :] + tm[i][..., None] * rays[i][1][:, None, :]
        x_s, x_t = (x_own, x_other) if i == 0 else (x_other, x_own)
        ds = ((x_s - torch.as_tensor(src["center"], dtype=torch.float32)) ** 2).sum(-1) + 1e-12
        dt_ = ((x_t - torch.as_tensor(tgt["center"], dtype=torch.float32)) ** 2).sum(-1) + 1e-12
        w_s = 1.0 / (1.0 + (ds / dt_) ** (0.5 * float(power)))
        w = w_s if i == 0 else 1.0 - w_s
        omega.append(torch.where(cov & occ[i] & bool(use_omega), w, torch.ones_like(w)))      # (lattice points that are not samples carry 1)
    alpha = [(1.0 - torch.exp(-(omega[i] * sigma[i]) * np.float32(blocks[i]["dt"]))) * occ[i] for i in (0, 1)]
    thre = [torch.full_like(tm[i], float(blocks[i].get("alpha_thre") or 0.0)) for i in (0, 1)]
    # merged stream: by t_mid, the source's sample first on a tie (stable sort of source-then-target); unmarched lattice points go last
    key = torch.cat([torch.where(occ[i], tm[i], torch.full_like(tm[i], float("inf"))) for i in (0, 1)], dim=1)
    order = torch.sort(key, dim=1, stable=True).indices
    cat = lambda parts: torch.gather(torch.cat(parts, dim=1), 1, order)
    is_src = cat([torch.ones_like(occ[0]), torch.zeros_like(occ[1])])
    t_m, occ_m, a_m, thre_m, om_m = cat(tm), cat(occ), cat(alpha), cat(thre), cat(omega)
    c_m = torch.gather(torch.cat(rgb_s, dim=1), 1, order[..., None].expand(-1, -1, 3))
    T_all = torch.cumprod(torch.cat([torch.ones(R, 1), 1.0 - a_m[:, :-1]], dim=1), dim=1)
    surv = occ_m & (T_all >= early_stop_eps) & ((thre_m <= 0) | (a_m >= thre_m))
    a_s = a_m * surv
    T_s = torch.cumprod(torch.cat([torch.ones(R, 1), 1.0 - a_s[:, :-1]], dim=1), dim=1)
    w = a_s * T_s
    opacity = w.sum(1)
    rgb = (w[..., None] * c_m).sum(1)
    if bkgd is not None:
        rgb = rgb + torch.as_tensor(bkgd, dtype=torch.float32) * (1.0 - opacity[:, None])
    return dict(rgb=rgb, opacity=opacity, depth=(w * t_m).sum(1), weight_src=(w * is_src).sum(1), n_samples=int(surv.sum()),
                is_src=is_src, t=t_m, omega=om_m, alpha=a_m, surv=surv)
