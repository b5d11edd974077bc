"""Point-to-plane ICP refinement of a predicted pose through the fused kernels of csrc/icp.hip: the "fine" half of the registration that the
reference states and never runs (refine_registration, conerf/geometry/global_registration.py:85-93; its call at :113 is commented out).
Rule: DESIGN.md §3f; CPU restatement: tests/icp_restatement.py.

The target cloud is indexed once (TargetIndex: a uniform grid of cells no narrower than the search radius, points sorted by cell — torch
plumbing); every iteration is then two launches (nearest neighbour + residuals + the 30 sums of the normal equations; 6x6 solve and pose
update) with the pose left on the device, and no host synchronisation until the caller reads the result."""
import math
from typing import Dict, Tuple

import torch

from . import lib as L

MAX_CELLS = 1 << 24
STATUS = {0: "running", 1: "converged", 2: "too_few", 3: "degenerate"}
STATS_COLUMNS = ("count", "sum_e2", "sum_d2", "norm_omega", "norm_v", "min_pivot_ratio", "status")


def default_cell(max_dist: float) -> float:
    """A cell width for searches up to max_dist.  The search is exact when a point within max_dist of q lies in the 27 cells around q's cell.  Cell
    indices are floor((x - lo) / cell) in fp32, a monotone function of x: its two roundings (2^-24 relative each) of a quotient below 2^12 (a grid
    of up to 4096 cells per axis) move an index across a cell face only for coordinates within 2^-11 cells of that face, so with a width of
    max_dist (1 + 2^-10) two points max_dist apart never land two faces apart.  With cell == max_dist exactly (allowed) the search is exact for every
    pair that is not within that rounding of the radius itself."""
    return float(max_dist) * (1.0 + 2.0 ** -10)


class TargetIndex:
    """Uniform-grid index of a target cloud: points fp32 [N,3] and normals fp32 [N,3] (a zero normal excludes its point) on one device.
    lo = min(points) - cell, dims_k = floor((max_k - lo_k) / cell) + 2 (one empty cell on every side), cell id = ix + nx (iy + ny iz) with
    ix = floor((x - lo_x) / cell) in fp32; points and normals are sorted stably by cell id (``perm`` = the caller's index of every sorted point),
    ``cell_start`` int32 [ncell + 1].  When the grid would have more than 2^24 cells, ``cell`` is doubled until it fits."""

    def __init__(self, points: torch.Tensor, normals: torch.Tensor, cell: float):
        if points.dim() != 2 or points.shape[1] != 3 or points.shape != normals.shape or points.shape[0] == 0:
            raise ValueError(f"TargetIndex: points {tuple(points.shape)} and normals {tuple(normals.shape)} must both be [N,3], N >= 1")
        if points.dtype != torch.float32 or normals.dtype != torch.float32:
            raise ValueError("TargetIndex: fp32 points and normals only")
        if points.device != normals.device:
            raise ValueError("TargetIndex: points and normals on different devices")
        if not (cell > 0.0 and math.isfinite(cell)):
            raise ValueError(f"TargetIndex: cell {cell} must be positive")
        if not bool(torch.isfinite(points).all()):
            raise ValueError("TargetIndex: non-finite point")
        points = points.contiguous()
        mn, mx = points.min(dim=0).values, points.max(dim=0).values
        cell32 = torch.tensor(float(cell), dtype=torch.float32)
        while True:
            c = cell32.to(points.device)
            lo = mn - c
            dims = [int(v) + 2 for v in torch.floor((mx - lo) / c).tolist()]
            if dims[0] * dims[1] * dims[2] <= MAX_CELLS:
                break
            cell32 = cell32 * 2
        key = torch.floor((points - lo) / c).long()
        cid = key[:, 0] + dims[0] * (key[:, 1] + dims[1] * key[:, 2])
        order = torch.sort(cid, stable=True).indices
        ncell = dims[0] * dims[1] * dims[2]
        counts = torch.bincount(cid, minlength=ncell)
        start = torch.zeros(ncell + 1, dtype=torch.int64, device=points.device)
        start[1:] = torch.cumsum(counts, dim=0)
        self.cell = float(cell32)
        self.lo = tuple(float(v) for v in lo.tolist())
        self.dims = tuple(dims)
        self.cell_id = cid                                   # per caller's point
        self.perm = order.to(torch.int32).contiguous()
        self.points = points[order].contiguous()
        self.normals = normals.contiguous()[order].contiguous()
        self.cell_start = start.to(torch.int32).contiguous()
        self.n = int(points.shape[0])
        self.device = points.device


def _pose12(pose: torch.Tensor, dev) -> torch.Tensor:
    if pose.shape[-2:] not in ((4, 4), (3, 4)) or pose.dim() != 2:
        raise ValueError(f"refine_pose: pose_init {tuple(pose.shape)} must be [4,4] or [3,4]")
    p = pose.detach().to(device=dev, dtype=torch.float64)
    return torch.cat([p[:3, :3].reshape(9), p[:3, 3]]).contiguous()


def refine_launch(src_pts: torch.Tensor, tgt_index: TargetIndex, pose12: torch.Tensor, max_dist: float, iters: int, tol_rot: float, tol_trans: float,
                  eps_cond: float = 1e-6, want_sums: bool = False, want_corr: bool = False) -> Dict[str, torch.Tensor]:
    """The C call: refines pose12 (fp64 [12] on the device) in place and returns the device tensors it wrote (stats [iters,7]; with want_sums the 30
    sums; with want_corr corr / dist2).  No host synchronisation."""
    if not src_pts.is_cuda or src_pts.device != tgt_index.device:
        raise ValueError("refine_pose: the source points and the target index must be on the same GPU (there is no CPU path)")
    if src_pts.dim() != 2 or src_pts.shape[1] != 3 or src_pts.dtype != torch.float32:
        raise ValueError(f"refine_pose: src_pts {tuple(src_pts.shape)} {src_pts.dtype} must be fp32 [Ns,3]")
    if not (max_dist >= 0.0) or tgt_index.cell < float(torch.tensor(float(max_dist), dtype=torch.float32)):      # compared in fp32, as the library does
        raise ValueError(f"refine_pose: the index's cell {tgt_index.cell} is narrower than max_dist {max_dist}: the 27-cell search would miss neighbours")
    if iters < 0:
        raise ValueError("refine_pose: iters < 0")
    src = src_pts.contiguous()
    ns = int(src.shape[0])
    dev = src.device
    lib = L.load()
    nbytes = lib.dreg_icp_workspace_bytes(ns, iters)
    out: Dict[str, torch.Tensor] = {}
    with torch.cuda.device(dev):
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        out["stats"] = torch.zeros(iters, 7, dtype=torch.float64, device=dev)
        if want_sums:
            out["sums"] = torch.zeros(30, dtype=torch.float64, device=dev)
        if want_corr:
            out["corr"] = torch.full((ns,), -1, dtype=torch.int32, device=dev)
            out["dist2"] = torch.full((ns,), float("inf"), dtype=torch.float32, device=dev)
        lo = (L.c_float * 3)(*tgt_index.lo)
        L.check(lib.dreg_icp_refine(L.ptr(src) if ns else None, ns, L.ptr(tgt_index.points), L.ptr(tgt_index.normals), L.ptr(tgt_index.perm),
                                    L.ptr(tgt_index.cell_start), tgt_index.n, lo, tgt_index.cell, tgt_index.dims[0], tgt_index.dims[1], tgt_index.dims[2],
                                    L.ptr(pose12), float(max_dist), iters, float(tol_rot), float(tol_trans), float(eps_cond),
                                    L.ptr(out["stats"]) if iters else None, L.ptr(out.get("sums")), L.ptr(out.get("corr")), L.ptr(out.get("dist2")),
                                    L.ptr(workspace), nbytes, L.stream()), "dreg_icp_refine")
        out["_workspace"] = workspace                        # alive until the caller drops the result (the launches are asynchronous)
    return out


def summarize(stats: torch.Tensor, ns: int) -> dict:
    """info of refine_pose from the stats table (a host copy): the last row that ran describes the run."""
    tab = stats.detach().cpu().double()
    iters = tab.shape[0]
    if iters == 0:
        return {"fitness": 0.0, "inlier_rmse": 0.0, "plane_rmse": 0.0, "iterations": 0, "status": 0, "stats": tab}
    st = tab[:, 6]
    nz = torch.nonzero(st != 0)
    done = int(nz[0]) + 1 if nz.numel() else iters
    row = tab[done - 1]
    count = float(row[0])
    return {"fitness": count / ns if ns else 0.0,
            "inlier_rmse": math.sqrt(float(row[2]) / count) if count > 0 else 0.0,
            "plane_rmse": math.sqrt(float(row[1]) / count) if count > 0 else 0.0,
            "iterations": done, "status": int(row[6]), "stats": tab}


def refine_pose(src_pts: torch.Tensor, tgt_index: TargetIndex, pose_init: torch.Tensor, max_dist: float = 0.05, iters: int = 30,
                tol_rot: float = 1e-7, tol_trans: float = 1e-7, eps_cond: float = 1e-6) -> Tuple[torch.Tensor, dict]:
    """Point-to-plane ICP from pose_init ([4,4], source -> target) against the indexed target: returns (pose fp64 [4,4] on the device, info).
    info: fitness = count / Ns, inlier_rmse = sqrt(sum d^2 / count), plane_rmse = sqrt(sum e^2 / count) (all three as of the last iteration that
    ran, before its update), iterations, status (1 converged, 0 ran out of iterations, 2 fewer than 6 correspondences, 3 degenerate system: with
    2 or 3 the returned pose is pose_init's), stats = the fp64 [iters,7] table (STATS_COLUMNS).  Reading info is the only host synchronisation."""
    dev = src_pts.device
    pose12 = _pose12(pose_init, dev)
    out = refine_launch(src_pts, tgt_index, pose12, max_dist, iters, tol_rot, tol_trans, eps_cond)
    pose = torch.zeros(4, 4, dtype=torch.float64, device=dev)
    pose[:3, :3] = pose12[:9].reshape(3, 3)
    pose[:3, 3] = pose12[9:]
    pose[3, 3] = 1.0
    return pose, summarize(out["stats"], int(src_pts.shape[0]))


def pca_normals(points: torch.Tensor, radius: float = 2 * 0.05, max_nn: int = 30, chunk: int = 2048) -> torch.Tensor:
    """fgr.estimate_normals (neighbourhood PCA, oriented away from the centroid) evaluated in row chunks: no N x N matrix is held."""
    n = points.shape[0]
    k = min(max_nn, n)
    centre = points.mean(dim=0)
    out = torch.empty_like(points)
    for a in range(0, n, chunk):
        rows = points[a:a + chunk]
        dist, idx = torch.topk(torch.cdist(rows, points).square(), k, dim=1, largest=False)
        nb = points[idx]
        w = (dist <= radius * radius).to(points.dtype)[..., None]
        cnt = w.sum(dim=1).clamp_min(1.0)
        mean = (nb * w).sum(dim=1) / cnt
        c = (nb - mean[:, None]) * w
        cov = c.transpose(1, 2) @ c / cnt[..., None]
        _, vec = torch.linalg.eigh(cov.double())
        nrm = vec[..., 0].to(points.dtype)
        sign = torch.where((nrm * (rows - centre)).sum(dim=1) < 0, -1.0, 1.0).to(points.dtype)
        out[a:a + chunk] = nrm * sign[:, None]
    return out


def block_normals(points: torch.Tensor, field=None) -> torch.Tensor:
    """Normals of a block's voxel point cloud for the ICP target: from the block's own density field when one is given (ngp.field_normals: the
    analytic gradient, no neighbourhood search), otherwise by PCA over the reference's FGR neighbourhood (radius 2 * 0.05, 30 neighbours)."""
    if field is not None:
        from . import ngp
        return ngp.field_normals(field, points)
    return pca_normals(points, 2 * 0.05, 30)


# ---------------------------------------------------------------------------------------------------------------- evaluator outputs
def refine_scene(src_pts: torch.Tensor, tgt_pts: torch.Tensor, pose_pred: torch.Tensor, pose_gt: torch.Tensor, tgt_field=None,
                 max_dist: float = 0.05, iters: int = 30, refiner=None, log=print, scene: str = ""):
    """eval_nerf_regtr.py --refine_pose for one scene: refine pose_pred ([1,3,4], the network's last layer) on the two voxel point clouds against
    the target's normals (tgt_field: the target block's field, else PCA — said in a printed line) and score it like the prediction.  Returns
    (row, pose [1,3,4]): row = the metrics row of ES.summary's schema with fitness, status and the refinement's time; a run that ends with status 2
    or 3 keeps the predicted pose.  refiner(src, index, pose4, max_dist=, iters=) -> (pose, info) defaults to refine_pose."""
    import time
    from . import losses as LS
    refiner = refine_pose if refiner is None else refiner
    if src_pts.is_cuda:
        torch.cuda.synchronize()
    t0 = time.time()
    if tgt_field is None:
        log(f"{scene}: target normals by PCA (no target block's field)")
    normals = block_normals(tgt_pts, tgt_field)
    index = TargetIndex(tgt_pts.contiguous(), normals.to(tgt_pts.dtype), default_cell(max_dist))
    p34 = pose_pred.reshape(3, 4)
    pose4 = torch.cat([p34, p34.new_tensor([[0.0, 0.0, 0.0, 1.0]])])
    pose, info = refiner(src_pts.contiguous(), index, pose4, max_dist=max_dist, iters=iters)
    if src_pts.is_cuda:
        torch.cuda.synchronize()
    dt = time.time() - t0
    out = pose_pred if info["status"] in (2, 3) else pose[:3].to(pose_pred.dtype).reshape(pose_pred.shape)
    err = LS.evaluate_camera_alignment(out, pose_gt)
    row = {"R_mean": float(err["R_error_mean"]), "t_mean": float(err["t_error_mean"]), "R_med": float(err["R_error_med"]), "t_med": float(err["t_error_med"]),
           "time": dt, "fitness": float(info["fitness"]), "status": int(info["status"])}
    return row, out


def write_refined_metrics(path: str, rows: dict) -> dict:
    """refined_metrics_{split}.json: ES.summary's layout (per-scene rows, R_mean / t_mean over the scenes), every row with fitness and status."""
    import json
    from . import eval_shard as ES
    out = ES.summary(rows)
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
    return out
