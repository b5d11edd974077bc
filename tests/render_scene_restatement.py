"""CPU restatement of the K-block renderer's rule (csrc/render_scene.hip), built on tests/render_restatement.py and
tests/render_pair_restatement.py: each block is marched on its own lattice exactly as the one-block rule marches it, the K sample streams are
merged by t_mid (the lowest block index first on a tie), a sample that other blocks cover as well is weighted by inverse distance to the blocks'
camera centroids, and the merged stream is composited by the one-block rule.  With K = 2 every operation is render_pair_restatement.render_pair's,
in its order: the results are equal, not close.

A block is the dict render_pair_restatement takes; rays are given per block, each in its own frame."""
import numpy as np
import torch

import render_pair_restatement as RP
import render_restatement as RR


def render_scene(blocks, rays, power=4.0, bkgd=None, early_stop_eps=1e-4, use_omega=True):
    """blocks: K dicts, rays: K pairs (o, d) [R,3] -> dict(rgb [R,3], opacity [R], depth [R], weight_block [R,K], n_samples int, and per merged
    sample [R, sum_b S_b], in composited order: block (index), t, omega, n_cover (other blocks covering it), alpha, surv)."""
    Kb = len(blocks)
    rays = [(o.float().cpu(), d.float().cpu()) for o, d in rays]
    R = rays[0][0].shape[0]
    tm, occ, sigma, rgb_s = [], [], [], []
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
    hp = 0.5 * float(power)
    center = [torch.as_tensor(b["center"], dtype=torch.float32) for b in blocks]
    omega, n_cover = [], []
    for i in range(Kb):
        x_own = rays[i][0][:, None, :] + tm[i][..., None] * rays[i][1][:, None, :]
        d_own = ((x_own - center[i]) ** 2).sum(-1) + 1e-12
        cnt = torch.zeros_like(tm[i], dtype=torch.long)
        ssum = torch.zeros_like(tm[i])
        w_pair = torch.ones_like(tm[i])
        for j in range(Kb):
            if j == i:
                continue
            cov, x_oth = RP.covered(blocks[j], rays[j][0], rays[j][1], tm[i])
            d_oth = ((x_oth - center[j]) ** 2).sum(-1) + 1e-12
            # the pair's rule between i and j: q = delta_lo / delta_hi, omega_lo = 1 / (1 + q^(p/2)), omega_hi = 1 - omega_lo
            d_lo, d_hi = (d_own, d_oth) if i < j else (d_oth, d_own)
            w_lo = 1.0 / (1.0 + (d_lo / d_hi) ** hp)
            w_ij = w_lo if i < j else 1.0 - w_lo
            w_pair = torch.where(cov & (cnt == 0), w_ij, w_pair)          # (used only where j stays the single covering block)
            ssum = ssum + torch.where(cov, (d_own / d_oth) ** hp, torch.zeros_like(ssum))
            cnt = cnt + cov.long()
        w = torch.where(cnt == 1, w_pair, 1.0 / (1.0 + ssum))
        omega.append(torch.where((cnt > 0) & occ[i] & bool(use_omega), w, torch.ones_like(w)))      # (lattice points that are not samples carry 1)
        n_cover.append(cnt * occ[i])
    alpha = [(1.0 - torch.exp(-(omega[i] * sigma[i]) * np.float32(blocks[i]["dt"]))) * occ[i] for i in range(Kb)]
    thre = [torch.full_like(tm[i], float(blocks[i].get("alpha_thre") or 0.0)) for i in range(Kb)]
    # merged stream: by t_mid, the lowest block index first on a tie (stable sort of the blocks in order); unmarched lattice points go last
    key = torch.cat([torch.where(occ[i], tm[i], torch.full_like(tm[i], float("inf"))) for i in range(Kb)], dim=1)
    order = torch.sort(key, dim=1, stable=True).indices
    cat = lambda parts: torch.gather(torch.cat(parts, dim=1), 1, order)
    blk = cat([torch.full_like(occ[i], i, dtype=torch.long) for i in range(Kb)])
    t_m, occ_m, a_m, thre_m, om_m, nc_m = cat(tm), cat(occ), cat(alpha), cat(thre), cat(omega), cat(n_cover)
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
    weight_block = torch.stack([(w * (blk == i)).sum(1) for i in range(Kb)], dim=1)
    return dict(rgb=rgb, opacity=opacity, depth=(w * t_m).sum(1), weight_block=weight_block, n_samples=int(surv.sum()),
                block=blk, t=t_m, omega=om_m, n_cover=nc_m, alpha=a_m, surv=surv)
