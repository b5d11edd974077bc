"""Joint point-to-plane ICP over a whole registered scene through the fused kernels of csrc/icp_scene.hip (CPU restatement:
tests/scene_icp_restatement.py): the residuals of ALL enabled ordered block pairs minimised over the K - 1 free poses at once, instead of
K (K - 1) pair refinements (icp.refine_pose) reconciled afterwards by a synchronisation that knows nothing of the geometry.

Every block is indexed once as a target (icp.TargetIndex over its own cloud and normals); an iteration is then two launches (the correspondence
rule of §3f for every pair in one grid; assembly, 6 (K - 1) Cholesky, pose update and the next relative poses in one workgroup) with the poses
left on the device, and no host synchronisation until the caller reads the result."""
import os
from typing import Dict, Sequence, Tuple

import torch

from . import icp
from . import lib as L

STATUS = icp.STATUS
STATS_COLUMNS = ("count", "sum_e2", "sum_d2", "max_norm_omega", "max_norm_v", "min_pivot_ratio", "status")


def _poses12(G: torch.Tensor, dev) -> torch.Tensor:
    if G.dim() != 3 or G.shape[-2:] not in ((4, 4), (3, 4)):
        raise ValueError(f"refine_poses: G_init {tuple(G.shape)} must be [K,4,4] or [K,3,4]")
    g = G.detach().to(device=dev, dtype=torch.float64)
    return torch.cat([g[:, :3, :3].reshape(-1, 9), g[:, :3, 3]], dim=1).contiguous()


def _mask_bytes(pair_mask, K: int):
    if pair_mask is None:
        return None, [(i, j) for i in range(K) for j in range(K) if i != j]
    m = torch.as_tensor(pair_mask).to("cpu")
    if tuple(m.shape) != (K, K):
        raise ValueError(f"refine_poses: pair_mask {tuple(m.shape)} must be [{K},{K}]")
    m = (m != 0).to(torch.uint8).contiguous()
    flat = m.reshape(-1).tolist()
    return (L.ctypes.c_uint8 * (K * K))(*flat), [(i, j) for i in range(K) for j in range(K) if i != j and flat[i * K + j]]


def refine_launch(points: Sequence[torch.Tensor], indices: Sequence[icp.TargetIndex], poses12: torch.Tensor, max_dist: float, iters: int,
                  tol_rot: float, tol_trans: float, eps_cond: float = 1e-6, pair_mask=None, want_pair_sums: bool = False,
                  want_rel: bool = False) -> Dict[str, torch.Tensor]:
    """The C call: refines poses12 (fp64 [K,12] on the device) in place and returns the device tensors it wrote (stats [iters,7]; with
    want_pair_sums the per-pair 30 sums [K,K,30]; with want_rel the relative poses [K,K,12]).  No host synchronisation."""
    K = len(points)
    if not 2 <= K <= L.SCENE_MAX_BLOCKS:
        raise ValueError(f"refine_poses: {K} blocks; a scene has 2 to {L.SCENE_MAX_BLOCKS}")
    if len(indices) != K or tuple(poses12.shape) != (K, 12):
        raise ValueError(f"refine_poses: {K} point clouds need {K} indices and poses [K,12]")
    dev = poses12.device
    if iters < 0:
        raise ValueError("refine_poses: iters < 0")
    md32 = float(torch.tensor(float(max_dist), dtype=torch.float32))
    srcs = []
    for b, (p, ix) in enumerate(zip(points, indices)):
        if not p.is_cuda or p.device != dev or ix.device != dev:
            raise ValueError("refine_poses: the points, the indices and the poses must be on the same GPU (there is no CPU path)")
        if p.dim() != 2 or p.shape[1] != 3 or p.dtype != torch.float32 or p.shape[0] < 1:
            raise ValueError(f"refine_poses: block {b}'s points {tuple(p.shape)} {p.dtype} must be fp32 [N,3], N >= 1")
        if ix.n != p.shape[0]:
            raise ValueError(f"refine_poses: block {b}'s index holds {ix.n} points, its cloud {p.shape[0]}: the index is over the block's own cloud")
        if not (max_dist >= 0.0) or ix.cell < md32:      # compared in fp32, as the library does
            raise ValueError(f"refine_poses: block {b}'s index has cell {ix.cell}, narrower than max_dist {max_dist}: the 27-cell search would miss neighbours")
        srcs.append(p.contiguous())
    blocks = (L.IcpBlock * K)()
    for b, (p, ix) in enumerate(zip(srcs, indices)):
        blocks[b].src, blocks[b].n = L.ptr(p), int(p.shape[0])
        blocks[b].tgt_points, blocks[b].tgt_normals, blocks[b].cell_start = L.ptr(ix.points), L.ptr(ix.normals), L.ptr(ix.cell_start)
        blocks[b].grid_lo = (L.c_float * 3)(*ix.lo)
        blocks[b].cell = ix.cell
        blocks[b].nx, blocks[b].ny, blocks[b].nz = ix.dims
    mask, pairs = _mask_bytes(pair_mask, K)
    lib = L.load()
    nbytes = lib.dreg_icp_scene_workspace_bytes(K, blocks, mask)
    out: Dict[str, torch.Tensor] = {}
    with torch.cuda.device(dev):
        workspace = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        out["stats"] = torch.zeros(iters, 7, dtype=torch.float64, device=dev)
        if want_pair_sums:
            out["pair_sums"] = torch.zeros(K, K, 30, dtype=torch.float64, device=dev)
        if want_rel:
            out["rel"] = torch.zeros(K, K, 12, dtype=torch.float64, device=dev)
        L.check(lib.dreg_icp_scene_refine(K, blocks, mask, L.ptr(poses12), float(max_dist), iters, float(tol_rot), float(tol_trans), float(eps_cond),
                                          L.ptr(out["stats"]) if iters else None, L.ptr(out.get("pair_sums")), L.ptr(out.get("rel")),
                                          L.ptr(workspace), nbytes, L.stream()), "dreg_icp_scene_refine")
        out["_workspace"] = workspace                        # alive until the caller drops the result (the launches are asynchronous)
        out["_srcs"] = srcs
    out["_pairs"] = pairs
    return out


def summarize(stats: torch.Tensor, n_src: int) -> dict:
    """info of refine_poses from the stats table (a host copy): icp.summarize with fitness over the source points of all enabled ordered pairs."""
    return icp.summarize(stats, n_src)


def refine_poses(points: Sequence[torch.Tensor], indices: Sequence[icp.TargetIndex], G_init: torch.Tensor, max_dist: float = 0.05, iters: int = 30,
                 tol_rot: float = 1e-7, tol_trans: float = 1e-7, eps_cond: float = 1e-6, pair_mask=None, want_pair_sums: bool = False,
                 want_rel: bool = False) -> Tuple[torch.Tensor, dict]:
    """Joint point-to-plane ICP of K blocks from G_init ([K,4,4], block b -> the anchor's frame; block 0 is the anchor and keeps its pose bit for
    bit): returns (G fp64 [K,4,4] on the device, info).  points[b]: block b's cloud fp32 [N_b,3] in its own frame; indices[b]: a TargetIndex over
    the same cloud with its normals, cell >= max_dist; pair_mask [K,K] (default all ones, diagonal ignored): ordered pair (i, j) = block i's points
    against block j's index.  info: status (1 converged, 0 ran out of iterations, 2 fewer than 6 (K - 1) correspondences, 3 degenerate system — e.g.
    a block with no correspondence to any other: with 2 or 3 the returned poses are G_init's), iterations, fitness = count / sum of N_i over the
    enabled ordered pairs, plane_rmse, inlier_rmse (as of the last iteration that ran, before its update), stats = the fp64 [iters,7] table
    (STATS_COLUMNS); with want_pair_sums / want_rel also the device tensors pair_sums [K,K,30] / rel [K,K,12].  Reading info is the only host
    synchronisation."""
    dev = points[0].device
    poses12 = _poses12(G_init, dev)
    out = refine_launch(points, indices, poses12, max_dist, iters, tol_rot, tol_trans, eps_cond, pair_mask, want_pair_sums, want_rel)
    K = len(points)
    G = torch.zeros(K, 4, 4, dtype=torch.float64, device=dev)
    G[:, :3, :3] = poses12[:, :9].reshape(K, 3, 3)
    G[:, :3, 3] = poses12[:, 9:]
    G[:, 3, 3] = 1.0
    info = summarize(out["stats"], sum(int(points[i].shape[0]) for i, _ in out["_pairs"]))
    for k in ("pair_sums", "rel"):
        if k in out:
            info[k] = out[k]
    return G, info


def block_points(block) -> torch.Tensor:
    """The voxel point cloud of one block of a scene list (scene_reg's block dicts), in the block's own frame: the occupied voxels' coordinates, as the
    evaluator reads them for a pair."""
    if "sparse" in block:
        return block["sparse"].vals[:, :3].float()
    g = block["xyz_rgba"]
    g = g.squeeze(0) if g.dim() == 6 else g
    m = block["mask"]
    m = m.squeeze(0) if m.dim() == 2 else m
    return g[:, :3].permute(0, 3, 4, 2, 1).reshape(-1, 3)[m].float()


def refine_registered_scene(scene, G_sync, device, max_dist: float = 0.05, iters: int = 30, normals: str = "field", log=print) -> Tuple[torch.Tensor, dict]:
    """--refine_scene for one scene: the synchronised poses G_sync [K,4,4] refined jointly on the blocks' voxel point clouds.  Normals from a
    block's own field when normals == "field" and its checkpoint is on disk, else by PCA (icp.block_normals; a printed line says so).  Returns
    (G fp64 [K,4,4] on the host, info); a run that ends with status 2 or 3 keeps G_sync."""
    pts, idx = [], []
    name = str(scene[0].get("scene", ""))
    for b, blk in enumerate(scene):
        p = block_points(blk).to(device).contiguous()
        field = None
        path = blk.get("nerf_path", "")
        if normals == "field" and path and os.path.exists(path):
            from .visibility import load_block
            field = load_block(path, device)[0]
            if field.unbounded:
                field = None
        if field is None:
            log(f"{name}: block {b}'s normals by PCA (no field of the block)")
        idx.append(icp.TargetIndex(p, icp.block_normals(p, field).to(p.dtype), icp.default_cell(max_dist)))
        pts.append(p)
    G0 = torch.as_tensor(G_sync).double()
    G, info = refine_poses(pts, idx, G0.to(device), max_dist=max_dist, iters=iters)
    return (G0.cpu() if info["status"] in (2, 3) else G.cpu()), info


def refined_scene_row(result: dict, G_refined, info: dict, scene) -> dict:
    """One scene's row of scene_refined_metrics_{split}.json: scene_reg.scene_row's schema for the refined poses, with status, iterations,
    fitness, and the synchronised R_mean / t_mean beside the refined ones.  Status 2 / 3 keep the synchronised poses."""
    from . import scene_reg
    kept = int(info["status"]) in (2, 3)
    sync = scene_reg.scene_row(result, scene)
    row = sync if kept else scene_reg.scene_row({**result, "G": torch.as_tensor(G_refined).double().cpu()}, scene)
    row = dict(row)
    row.update({"status": int(info["status"]), "iterations": int(info["iterations"]), "fitness": float(info["fitness"]),
                "R_mean_sync": sync["R_mean"], "t_mean_sync": sync["t_mean"]})
    return row


def write_scene_refined_metrics(path: str, rows: dict) -> dict:
    """scene_refined_metrics_{split}.json: scene_reg.summary's layout plus the means of the synchronised errors."""
    import json
    from . import scene_reg
    out = scene_reg.summary(rows)
    for k in ("R_mean_sync", "t_mean_sync"):
        out[k] = sum(r[k] for r in rows.values()) / max(len(rows), 1)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
    return out
