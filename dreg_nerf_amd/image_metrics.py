"""PSNR and SSIM of rendered views against their ground truth through the fused kernel of csrc/image_metrics.hip: the arithmetic of the
reference's evaluate() (eval_ngp_nerf.py:24-31,214-229; conerf/loss/ssim_torch.py) for a batch of views in one call, every result left on the
device.  Rule: DESIGN.md §3d; CPU restatement: tests/image_metrics_restatement.py.  LPIPS is not computed (no network weights in this project).

Also here, because the evaluator writes them from these results: the metrics.json writer and the depth-range point selection of the reference's
generate_point_cloud (eval_ngp_nerf.py:246-334)."""
import ctypes
import json
import math
from typing import Dict, List, Sequence

import torch

from . import lib as L

WINDOW_SIZE = 11
SIGMA = 1.5
EPS = 1e-6


def gaussian_taps(window_size: int = WINDOW_SIZE, sigma: float = SIGMA) -> torch.Tensor:
    """The window's 1-D taps as ssim_torch.gaussian forms them: Python floats -> fp32 -> divided by their fp32 sum."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    return g / g.sum()


_TAPS = None


def _taps_c():
    global _TAPS
    if _TAPS is None:
        _TAPS = (ctypes.c_float * WINDOW_SIZE)(*gaussian_taps().tolist())
    return _TAPS


def image_metrics(pred: torch.Tensor, gt: torch.Tensor, return_map: bool = False, return_u8: bool = False) -> Dict[str, torch.Tensor]:
    """pred, gt: fp32 [H,W,C] or [N,H,W,C] on the device, channel-last, 1 <= C <= 4 (made contiguous when they are not).  Returns device tensors:
    ssim, mse, psnr fp32 [N]; with return_map ssim_map fp32 [N,H,W,C]; with return_u8 pred_u8 / gt_u8 uint8 [N,H,W,C] =
    (v.clamp(0, 1) * 255).to(uint8).  No host synchronisation.  Not differentiable: raises when an input requires grad."""
    if pred.requires_grad or gt.requires_grad:
        raise RuntimeError("image_metrics: the fused metrics kernel has no backward; detach the images or call it under torch.no_grad()")
    if pred.shape != gt.shape or pred.dim() not in (3, 4):
        raise ValueError(f"image_metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must both be [H,W,C] or [N,H,W,C]")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError("image_metrics: fp32 images only")
    if not pred.is_cuda or pred.device != gt.device:
        raise ValueError("image_metrics: both images must be on the same GPU (there is no CPU path)")
    if pred.dim() == 3:
        pred, gt = pred[None], gt[None]
    pred, gt = pred.contiguous(), gt.contiguous()
    n, h, w, c = pred.shape
    lib = L.load()
    nbytes = lib.dreg_image_metrics_workspace_bytes(n, h, w, c)
    if nbytes == 0:
        raise ValueError(f"image_metrics: unsupported shape {tuple(pred.shape)} (N <= 65535, H, W >= 1, 1 <= C <= 4)")
    dev = pred.device
    with torch.cuda.device(dev):
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        res = torch.empty(3, n, dtype=torch.float32, device=dev)
        out = {"ssim": res[0], "mse": res[1], "psnr": res[2]}
        if return_map:
            out["ssim_map"] = torch.empty_like(pred)
        if return_u8:
            out["pred_u8"] = torch.empty(pred.shape, dtype=torch.uint8, device=dev)
            out["gt_u8"] = torch.empty(pred.shape, dtype=torch.uint8, device=dev)
        L.check(lib.dreg_image_metrics(L.ptr(pred), L.ptr(gt), n, h, w, c, _taps_c(), L.ptr(out["ssim"]), L.ptr(out["mse"]), L.ptr(out["psnr"]),
                                       L.ptr(out.get("ssim_map")), L.ptr(out.get("pred_u8")), L.ptr(out.get("gt_u8")),
                                       L.ptr(workspace), nbytes, L.stream()), "dreg_image_metrics")
    return out


def _nchw_pair(gt_image: torch.Tensor, pred_image: torch.Tensor):
    if gt_image.dim() != 4 or gt_image.shape[0] != 1 or gt_image.shape != pred_image.shape:
        raise ValueError(f"expected two [1,C,H,W] images, got {tuple(gt_image.shape)} and {tuple(pred_image.shape)}")
    return pred_image.permute(0, 2, 3, 1), gt_image.permute(0, 2, 3, 1)


def compute_psnr(gt_image: torch.Tensor, pred_image: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """The reference's compute_psnr (eval_ngp_nerf.py:24-27): [1,C,H,W] images -> 0-dim tensor -10 ln(mse + eps) / ln 10."""
    pred, gt = _nchw_pair(gt_image, pred_image)
    m = image_metrics(pred, gt)
    if eps == EPS:
        return m["psnr"][0]
    return -10.0 * torch.log(m["mse"][0] + eps) / math.log(10.0)


def compute_ssim(gt_image: torch.Tensor, pred_image: torch.Tensor) -> float:
    """The reference's compute_ssim (eval_ngp_nerf.py:30-31): [1,C,H,W] images -> the mean SSIM as a Python float."""
    pred, gt = _nchw_pair(gt_image, pred_image)
    return image_metrics(pred, gt)["ssim"][0].item()


# ---------------------------------------------------------------------------------------------------------------- evaluator outputs
def metrics_dict(scene: str, psnrs: Sequence[float], ssims: Sequence[float]) -> dict:
    """metrics.json of the reference's evaluate() (eval_ngp_nerf.py:226-238) without the lpips keys:
    {scene: {"0": {"psnr", "ssim"}, ..., "psnr": mean, "ssim": mean}}."""
    if len(psnrs) != len(ssims) or len(psnrs) == 0:
        raise ValueError("metrics_dict: one psnr and one ssim per view, at least one view")
    rows = {str(i): {"psnr": float(p), "ssim": float(s)} for i, (p, s) in enumerate(zip(psnrs, ssims))}
    rows["psnr"] = sum(float(p) for p in psnrs) / len(psnrs)
    rows["ssim"] = sum(float(s) for s in ssims) / len(ssims)
    return {scene: rows}


def write_metrics_json(path: str, scene: str, psnrs: Sequence[float], ssims: Sequence[float]) -> dict:
    d = metrics_dict(scene, psnrs, ssims)
    with open(path, "w") as f:
        f.write(json.dumps(d, indent=4))
    return d


def select_depth_points(origins: torch.Tensor, viewdirs: torch.Tensor, depth: torch.Tensor, rgb: torch.Tensor,
                        min_depth: float = 2.0, max_depth: float = 6.0):
    """One camera's share of generate_point_cloud (eval_ngp_nerf.py:308-320): the pixels with min_depth <= depth <= max_depth, in pixel order,
    as (points = o + d * depth [M,3], colours [M,3])."""
    o, d, rgb = origins.reshape(-1, 3), viewdirs.reshape(-1, 3), rgb.reshape(-1, 3)
    z = depth.reshape(-1, 1)
    keep = (z[:, 0] <= max_depth) & (z[:, 0] >= min_depth)
    return o[keep] + d[keep] * z[keep], rgb[keep]


def point_cloud_from_views(views, min_depth: float = 2.0, max_depth: float = 6.0):
    """views: an iterable of (origins, viewdirs, depth, rgb) per camera -> (points [M,3], colours [M,3]) in camera-then-pixel order."""
    pts: List[torch.Tensor] = []
    cols: List[torch.Tensor] = []
    for o, d, z, rgb in views:
        p, c = select_depth_points(o, d, z, rgb, min_depth, max_depth)
        pts.append(p)
        cols.append(c)
    return torch.cat(pts, dim=0), torch.cat(cols, dim=0)
