"""Robust pose from the network's predicted correspondences through the fused kernels of csrc/pose_ransac.hip: thousands of minimal-sample
hypotheses scored against all correspondences in one launch, the best one selected on the device, then consensus refits with the existing
weighted Kabsch solve.  Rule: DESIGN.md §3g; CPU restatement: tests/pose_ransac_restatement.py.

The single weighted Kabsch solve that gives pred["pose"] has no notion of an outlier: correspondences that fall into two self-consistent groups
give a blend of the two motions.  This estimator returns the motion of the larger group.  Whether it moves the three near-symmetric scenes of
the trained-regime record is NOT measured (no trained checkpoint is at hand); the threshold default 0.05 (round 0's voxel-average cell, ICP's
default gate) is NOT tuned."""
from typing import Dict, Optional, Tuple

import torch

from . import attn_ops as A
from . import lib as L

STATUS = {0: "found", 2: "no_valid_hypothesis"}


def correspondences(pred: dict, layer: int = -1, min_overlap: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(a, b, w) of one pair's prediction, both directions stacked as NeRFRegTr.forward stacks them for its Kabsch solve:
    a = [src_kp ; tgt_kp_warped[layer]], b = [src_kp_warped[layer] ; tgt_kp], w = [src_overlap[layer] ; tgt_overlap[layer]]; rows with
    w < min_overlap are dropped."""
    s_xyz, t_xyz = pred["src_kp"][0], pred["tgt_kp"][0]
    s_corr, t_corr = pred["src_kp_warped"][0][layer], pred["tgt_kp_warped"][0][layer]
    s_ov, t_ov = pred["src_overlap"][0][layer], pred["tgt_overlap"][0][layer]
    a = torch.cat([s_xyz, t_corr]).detach().float()
    b = torch.cat([s_corr, t_xyz]).detach().float()
    w = torch.cat([s_ov.reshape(-1), t_ov.reshape(-1)]).detach().float()
    if min_overlap > 0.0:
        keep = w >= min_overlap
        a, b, w = a[keep], b[keep], w[keep]
    return a.contiguous(), b.contiguous(), w.contiguous()


def _check(a, b, name):
    if not a.is_cuda or a.device != b.device:
        raise ValueError(f"{name}: a and b must be on the same GPU (there is no CPU path)")
    if a.dim() != 2 or a.shape[1] != 3 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"{name}: a {tuple(a.shape)} {a.dtype} and b {tuple(b.shape)} {b.dtype} must both be fp32 [N,3]")


def ransac_launch(a: torch.Tensor, b: torch.Tensor, triplets: torch.Tensor, thresh: float, eps_area: float = 1e-4, pose: Optional[torch.Tensor] = None,
                  want_counts: bool = False, want_poses: bool = False) -> Dict[str, torch.Tensor]:
    """The C call: scores every triplet and selects.  Returns the device tensors it wrote: best int32 [2], pose fp32 [12] (the given buffer, or one
    filled with the identity; untouched with status 2), status int32 [1], mask uint8 [N]; with want_counts / want_poses the per-hypothesis
    tables.  No host synchronisation."""
    _check(a, b, "ransac_launch")
    if triplets.dim() != 2 or triplets.shape[1] != 3 or triplets.dtype != torch.int32 or triplets.device != a.device or triplets.shape[0] == 0:
        raise ValueError(f"ransac_launch: triplets {tuple(triplets.shape)} {triplets.dtype} must be int32 [H,3], H >= 1, on the points' device")
    a, b, triplets = a.contiguous(), b.contiguous(), triplets.contiguous()
    n, h, dev = int(a.shape[0]), int(triplets.shape[0]), a.device
    lib = L.load()
    nbytes = lib.dreg_pose_ransac_workspace_bytes(n, h)
    out: Dict[str, torch.Tensor] = {}
    with torch.cuda.device(dev):
        workspace = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=dev)
        out["best"] = torch.empty(2, dtype=torch.int32, device=dev)
        out["status"] = torch.empty(1, dtype=torch.int32, device=dev)
        if pose is None:
            pose = torch.cat([torch.eye(3, dtype=torch.float32, device=dev).reshape(9), torch.zeros(3, dtype=torch.float32, device=dev)])
        out["pose"] = pose
        out["mask"] = torch.zeros(n, dtype=torch.uint8, device=dev)
        if want_counts:
            out["counts"] = torch.empty(h, dtype=torch.int32, device=dev)
        if want_poses:
            out["poses"] = torch.empty(h, 12, dtype=torch.float32, device=dev)
        L.check(lib.dreg_pose_ransac(L.ptr(a) if n else None, L.ptr(b) if n else None, n, L.ptr(triplets), h, float(thresh), float(eps_area), L.ptr(workspace),
                                     nbytes, L.ptr(out["best"]), L.ptr(pose), L.ptr(out["status"]), L.ptr(out.get("counts")), L.ptr(out.get("poses")),
                                     L.ptr(out["mask"]) if n else None, L.stream()), "dreg_pose_ransac")
        out["_workspace"] = workspace                        # alive until the caller drops the result (the launches are asynchronous)
    return out


def pose_inliers(a: torch.Tensor, b: torch.Tensor, pose12: torch.Tensor, thresh: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """mask uint8 [N] and count int32 [1] of a pose fp32 [12] (R row-major, then t) on the device.  No host synchronisation."""
    _check(a, b, "pose_inliers")
    if pose12.shape != (12,) or pose12.dtype != torch.float32 or pose12.device != a.device:
        raise ValueError("pose_inliers: pose must be fp32 [12] on the points' device")
    a, b, pose12 = a.contiguous(), b.contiguous(), pose12.contiguous()
    n = int(a.shape[0])
    with torch.cuda.device(a.device):
        mask = torch.zeros(n, dtype=torch.uint8, device=a.device)
        count = torch.zeros(1, dtype=torch.int32, device=a.device)
        L.check(L.load().dreg_pose_inliers(L.ptr(a) if n else None, L.ptr(b) if n else None, n, L.ptr(pose12), float(thresh), L.ptr(mask) if n else None,
                                           L.ptr(count), L.stream()), "dreg_pose_inliers")
    return mask, count


def draw_triplets(n: int, hyps: int, seed: int, device) -> torch.Tensor:
    """int32 [hyps,3] drawn on the device from a generator seeded by `seed` (rows with a repeated index are invalid hypotheses, not redrawn)."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return torch.randint(0, max(n, 1), (hyps, 3), generator=g, device=device, dtype=torch.int32)


def estimate_pose(a: torch.Tensor, b: torch.Tensor, w: Optional[torch.Tensor] = None, thresh: float = 0.05, hyps: int = 16384, lo_iters: int = 3,
                  seed: int = 0, triplets: Optional[torch.Tensor] = None, eps_area: float = 1e-4) -> Tuple[torch.Tensor, dict]:
    """Pose (fp32 [3,4] on the device, source -> target) with the largest consensus among the correspondences a[i] -> b[i], and info.

    Minimal stage: `hyps` triplets (drawn on the device from `seed` unless given), each scored by its inlier count at `thresh`; the best one's pose
    is the minimal pose.  Then lo_iters rounds, unconditionally: pose <- weighted_kabsch(a, b, w * mask(pose)); mask, count <- inliers(pose).
    The returned pose is that of the last round whose fitted set had >= 3 members and whose result is finite, else the minimal pose; with status 2
    (no valid hypothesis) it is the identity and the caller keeps whatever pose it had.  Every launch is enqueued without a host decision; reading
    info is the one readback.  info: status, inliers / inlier_ratio (of the returned pose), best_index, minimal_pose [3,4], minimal_inliers,
    round_inliers (count after each round), round_used (-1 = the minimal pose).  Two calls with the same arguments are bit-identical."""
    _check(a, b, "estimate_pose")
    n, dev = int(a.shape[0]), a.device
    if w is None:
        w = torch.ones(n, dtype=torch.float32, device=dev)
    if w.shape != (n,) or w.device != dev:
        raise ValueError(f"estimate_pose: w {tuple(w.shape)} must be [N] on the points' device")
    if lo_iters < 0 or hyps < 1:
        raise ValueError("estimate_pose: lo_iters < 0 or hyps < 1")
    w = w.detach().float().contiguous()
    a, b = a.contiguous(), b.contiguous()
    if triplets is None:
        triplets = draw_triplets(n, hyps, seed, dev)
    out = ransac_launch(a, b, triplets, thresh, eps_area)
    minimal, mask = out["pose"], out["mask"]
    count = out["best"][1:2]
    cur, used = minimal, torch.full((1,), -1, dtype=torch.int32, device=dev)
    final_count = count
    poses, counts = [minimal], [count]
    for r in range(lo_iters):
        fitted = count
        p34 = A.weighted_kabsch(a[None], b[None], (w * mask.to(torch.float32))[None])[0]
        p12 = torch.cat([p34[:, :3].reshape(9), p34[:, 3]]).contiguous()
        mask, count = pose_inliers(a, b, p12, thresh)
        ok = (fitted >= 3) & torch.isfinite(p12).all() & (out["status"] == 0)
        cur = torch.where(ok, p12, cur)
        used = torch.where(ok, torch.full_like(used, r), used)
        final_count = torch.where(ok, count, final_count)
        poses.append(p12)
        counts.append(count)
    # one readback: the integers and the bit patterns of the poses in one int32 table
    table = torch.cat([out["best"], out["status"], used, final_count, torch.cat(counts), torch.stack(poses + [cur]).reshape(-1).view(torch.int32)]).cpu()
    ints = table[:5 + len(counts)].tolist()
    fl = table[5 + len(counts):].view(torch.float32).reshape(len(poses) + 1, 12)

    def p34_of(p12):
        return torch.cat([p12[:9].reshape(3, 3), p12[9:].reshape(3, 1)], dim=1)

    info = {"status": ints[2], "inliers": ints[4], "inlier_ratio": ints[4] / n if n else 0.0, "best_index": ints[0], "minimal_pose": p34_of(fl[0]),
            "minimal_inliers": ints[1], "round_inliers": ints[6:], "round_used": ints[3], "round_poses": [p34_of(p) for p in fl[1:-1]], "hyps": int(triplets.shape[0])}
    return p34_of(cur), info


# ---------------------------------------------------------------------------------------------------------------- evaluator outputs
def ransac_scene(pred: dict, pose_gt: torch.Tensor, thresh: float = 0.05, hyps: int = 16384, seed: int = 0, min_overlap: float = 0.0, estimator=None):
    """eval_nerf_regtr.py --ransac_pose for one scene: the pose estimated from the last layer's correspondences, scored like the prediction.  Returns
    (row, pose [1,3,4]): row = the metrics row of ES.summary's schema plus inliers, inlier_ratio and status; a scene with status 2 keeps the
    predicted pose.  estimator(a, b, w, thresh=, hyps=, seed=) -> (pose [3,4], info) defaults to estimate_pose."""
    import time
    from . import losses as LS
    estimator = estimate_pose if estimator is None else estimator
    a, b, w = correspondences(pred, -1, min_overlap)
    if a.is_cuda:
        torch.cuda.synchronize()
    t0 = time.time()
    pose, info = estimator(a, b, w, thresh=thresh, hyps=hyps, seed=seed)
    if a.is_cuda:
        torch.cuda.synchronize()
    dt = time.time() - t0
    pose_pred = pred["pose"][-1]
    out = pose_pred if info["status"] == 2 else pose.to(device=pose_pred.device, dtype=pose_pred.dtype).reshape(pose_pred.shape)
    err = LS.evaluate_camera_alignment(out, pose_gt)
    row = {"R_mean": float(err["R_error_mean"]), "t_mean": float(err["t_error_mean"]), "R_med": float(err["R_error_med"]), "t_med": float(err["t_error_med"]),
           "time": dt, "inliers": int(info["inliers"]), "inlier_ratio": float(info["inlier_ratio"]), "status": int(info["status"])}
    return row, out


def write_ransac_metrics(path: str, rows: dict) -> dict:
    """ransac_metrics_{split}.json: ES.summary's layout (per-scene rows, R_mean / t_mean over the scenes), every row with inliers, inlier_ratio, status."""
    import json
    from . import eval_shard as ES
    out = ES.summary(rows)
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
    return out
