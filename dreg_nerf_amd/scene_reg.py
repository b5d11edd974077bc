"""Registration of a WHOLE scene: all K (K - 1) ordered pairs of a scene's blocks through the network, the predicted poses
synchronised into one pose per block (pose_graph.synchronize), and the rows of scene_metrics_{split}.json.

A scene is the list NeRFRegDataset.get_scene / synth.shell_scene return: block dicts ordered by id with `sparse` (SparseBlock) or `xyz_rgba` and
`mask`, `nerf_path`, `transform`.  The anchor is the first block (the lowest id); G_i maps block i's frame to the anchor's, and the ground truth
is transform[anchor] @ inv(transform[i])."""
import json
import os

import numpy as np
import torch

from . import losses as LS
from . import pose_graph


def pair_sample(scene, i, j, device=None):
    """Blocks i (source) and j (target) of a scene as the sample NeRFRegDataset.get returns for that pair (never augmented)."""
    s, t = scene[i], scene[j]
    data = {"src_nerf_path": s.get("nerf_path", ""), "tgt_nerf_path": t.get("nerf_path", ""),
            "pose": (t["transform"].float() @ torch.linalg.inv(s["transform"].float()))[None], "block_list": [s.get("block_id", i), t.get("block_id", j)]}
    for side, b in (("src", s), ("tgt", t)):
        if "sparse" in b:
            data[side + "_sparse"] = b["sparse"]
        else:
            data[side + "_xyz_rgba"], data[side + "_mask"] = b["xyz_rgba"], b["mask"]
    for k in ("scene", "dataset", "index"):
        if k in s:
            data[k] = s[k]
    if device is not None:
        data = {k: (v.to(device) if torch.is_tensor(v) or hasattr(v, "idx") else v) for k, v in data.items()}
    return data


def ground_truth(scene) -> torch.Tensor:
    """G [K,4,4] fp64: block i's frame -> the anchor's (block 0 of the list)."""
    T = [b["transform"].double().cpu() for b in scene]
    return torch.stack([T[0] @ torch.linalg.inv(Ti) for Ti in T])


def register_scene(model, scene, robust=False, pair_fn=None, eval_batch=4, device=None, c_rot_deg=2.0, c_trans=0.05, iters=10) -> dict:
    """All ordered pairs (i, j), i != j, through model.forward_batch in batches of eval_batch; edge (i, j) is pred["pose"][-1] (frame i -> frame j)
    with weight 1.  pair_fn(i, j, sample) -> pose ([3,4] or [4,4]) replaces the network (tests; the hook for ICP- or RANSAC-refined edges).
    Returns G [K,4,4] fp64 (torch, host), edges: [{i, j, pose [4,4] as lists}] in (i, j) order, info: pose_graph.synchronize's, as lists."""
    K = len(scene)
    pairs = [(i, j) for i in range(K) for j in range(K) if i != j]
    poses = []
    if pair_fn is not None:
        poses = [pair_fn(i, j, pair_sample(scene, i, j, device)) for i, j in pairs]
    else:
        if device is None:
            device = next(model.parameters()).device
        with torch.no_grad():
            for b0 in range(0, len(pairs), max(int(eval_batch), 1)):
                batch = [pair_sample(scene, i, j, device) for i, j in pairs[b0:b0 + max(int(eval_batch), 1)]]
                poses += [pred["pose"][-1][0] for pred in model.forward_batch(batch)]
                if hasattr(model, "check_inputs"):
                    model.check_inputs()      # as the evaluator's normal pass: a grid with values outside its voxel_mask is an error of THESE blocks
    P = [pose_graph._pose44(p) for p in poses]
    G, info = pose_graph.synchronize(K, [(i, j, p, 1.0) for (i, j), p in zip(pairs, P)], anchor=0, robust=robust, c_rot_deg=c_rot_deg, c_trans=c_trans, iters=iters)
    return {"G": torch.from_numpy(G), "edges": [{"i": i, "j": j, "pose": p.tolist()} for (i, j), p in zip(pairs, P)],
            "info": {k: [float(x) for x in v] for k, v in info.items()}}


def _errors(G, G_gt):
    e = LS.evaluate_camera_alignment(torch.as_tensor(G)[None, :3].float(), torch.as_tensor(G_gt)[None].float())
    return float(e["R_error_mean"]), float(e["t_error_mean"])


def scene_row(result: dict, scene) -> dict:
    """One scene's row of scene_metrics_{split}.json: per block the RRE (degrees) / RTE of the synchronised G_i against the ground truth and,
    beside it, of the direct edge i -> anchor (what a pairwise run would have given); per edge its residual and final weight; the means."""
    G_gt = ground_truth(scene)
    direct = {e["i"]: torch.tensor(e["pose"], dtype=torch.float64) for e in result["edges"] if e["j"] == 0}
    blocks = []
    for i in range(len(scene)):
        rre, rte = (0.0, 0.0) if i == 0 else _errors(result["G"][i], G_gt[i])
        rre_d, rte_d = (0.0, 0.0) if i == 0 else _errors(direct[i], G_gt[i])
        blocks.append({"block": scene[i].get("block_id", i), "rre": rre, "rte": rte, "rre_direct": rre_d, "rte_direct": rte_d})
    info = result["info"]
    edges = [{"i": e["i"], "j": e["j"], "residual_rot_deg": info["residual_rot_deg"][k], "residual_trans": info["residual_trans"][k], "weight": info["weights"][k]}
             for k, e in enumerate(result["edges"])]
    others = blocks[1:] or blocks
    mean = lambda key: float(np.mean([b[key] for b in others]))
    return {"blocks": blocks, "edges": edges, "R_mean": mean("rre"), "t_mean": mean("rte"), "R_mean_direct": mean("rre_direct"), "t_mean_direct": mean("rte_direct")}


def summary(rows: dict) -> dict:
    """scene_metrics_{split}.json: the per-scene rows and, in eval_shard.summary's style, the means over the scenes (synchronised and direct)."""
    out = dict(rows)
    for k in ("R_mean", "t_mean", "R_mean_direct", "t_mean_direct"):
        out[k] = sum(r[k] for r in rows.values()) / max(len(rows), 1)
    return out


def write_scene_metrics(path: str, rows: dict) -> dict:
    out = summary(rows)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
    return out


def render_registered_scene(output_dir: str, scene, G_gt, G_sync, dataset: str, device, renderer=None, metrics=None) -> dict:
    """--render_scene for one scene: all blocks rendered as ONE scene (render.render_blocks_views) from every block's cameras, brought into the
    anchor frame by the ground-truth poses, under the ground-truth G (prefix gt) and the synchronised G (prefix aligned):
    {prefix}_scene_images/rgb_i.png, depth_i.png and share_b_i.png (block b's share of the opacity, grey).  scene_render_metrics.json holds PSNR /
    SSIM of the aligned views against the gt views, from ONE image_metrics call.  renderer(poses [K,4,4], poses_c2w, K, W, H) -> (rgbs, depths,
    shares [H,W,K]) and metrics(aligned_rgbs, gt_rgbs) -> (psnrs, ssims) may be injected (tests)."""
    from . import render as R
    Kc, W, H = R.intrinsics(dataset)
    paths = [b["nerf_path"] for b in scene]
    if renderer is None:
        loaded = [R.load_render_block(p, device) for p in paths]
        cams = [b[2]["camera_poses"] for b in loaded]

        def renderer(poses, poses_c2w, K_, W_, H_):
            return R.render_blocks_views(loaded, poses, poses_c2w, K_, W_, H_)
    else:
        cams = [R.block_camera_poses(p) for p in paths]
    metrics = metrics or R._stack_metrics
    G_gt, G_sync = torch.as_tensor(G_gt).double().cpu(), torch.as_tensor(G_sync).double().cpu()
    views = torch.cat([(G_gt[b] @ torch.as_tensor(cams[b]).double().cpu()).float() for b in range(len(scene))], dim=0)
    os.makedirs(output_dir, exist_ok=True)
    stacks = {}
    for prefix, G in (("gt", G_gt), ("aligned", G_sync)):
        rgbs, depths, shares = renderer(G, views, Kc, W, H)
        stacks[prefix] = rgbs
        d = os.path.join(output_dir, prefix + "_scene_images")
        os.makedirs(d, exist_ok=True)
        for i in range(len(rgbs)):
            rgb, depth, share = (np.asarray(v.cpu() if torch.is_tensor(v) else v) for v in (rgbs[i], depths[i], shares[i]))
            R._png(os.path.join(d, f"rgb_{i}.png"), rgb)
            R._png(os.path.join(d, f"depth_{i}.png"), R.colorize_depth(depth.squeeze(-1)))
            for b in range(len(scene)):
                R._png(os.path.join(d, f"share_{b}_{i}.png"), np.repeat(share.reshape(H, W, -1)[:, :, b:b + 1], 3, axis=2))
    psnr, ssim = metrics(stacks["aligned"], stacks["gt"])
    out = {"views": [{"psnr": float(p), "ssim": float(s)} for p, s in zip(psnr, ssim)], "psnr_mean": float(np.mean(psnr)), "ssim_mean": float(np.mean(ssim))}
    with open(os.path.join(output_dir, "scene_render_metrics.json"), "w") as f:
        json.dump(out, f, indent=2)
    return out
