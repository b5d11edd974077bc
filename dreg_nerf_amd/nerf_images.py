"""Posed RGBA images of one NeRF training scene: the reference's SubjectLoader for `objaverse` and `nerf_synthetic`
(conerf/datasets/{objaverse,nerf_synthetic,dataset_base}.py) as train_ngp_nerf.py reads them.

  objaverse       <root>/<scene>/transforms.json, frames i % 20 == 0 are the test split, the rest train
  nerf_synthetic  <root>/<scene>/transforms_{split}.json
  --multi_blocks  KMeans(n_clusters, random_state=0, n_init="auto") on the camera centres (conerf/register/cluster.py), then the every-20th
                  test split inside each block

Pixels are RGBA composited over a white background (rgb a + (1 - a)); the focal length comes from camera_angle_x and the principal point is the
image centre (the reference writes WIDTH / 2 = 400 for its 800 x 800 renders).  `factor` is accepted and, as in the reference's objaverse loader,
not applied.  The images stay on the device and ray batches are drawn there."""
import json
import math
import os
from typing import List, Optional

import numpy as np
import torch

from .render import Rays

VAL_INTERVAL = 20
DATASETS = ("objaverse", "nerf_synthetic")


def _read_png(path: str) -> np.ndarray:
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGBA"))
    return img


def block_labels(camtoworlds: np.ndarray, num_blocks: int) -> np.ndarray:
    """Camera-cluster label of every view: sklearn KMeans on the camera centres (conerf/register/cluster.py)."""
    from sklearn.cluster import KMeans
    return KMeans(n_clusters=num_blocks, random_state=0, n_init="auto").fit(camtoworlds[:, :3, -1]).labels_


def _split_every_20(ids: np.ndarray, split: str) -> np.ndarray:
    pos = np.arange(ids.shape[0])
    return ids[pos % VAL_INTERVAL == 0] if split == "test" else ids[pos % VAL_INTERVAL != 0]


def load_renderings(dataset: str, root_dir: str, scene: str, split: str, multi_blocks: bool = False, num_blocks: int = 1):
    """(images uint8 [N,H,W,4] or a list of them per block, camtoworlds fp32 [N,4,4] or a list, focal) of one scene's split."""
    if dataset not in DATASETS:
        raise NotImplementedError(f"NeRF training reads {DATASETS}, not {dataset!r}")
    data_dir = os.path.join(root_dir, scene)
    meta_name = "transforms.json" if dataset == "objaverse" else f"transforms_{split}.json"
    with open(os.path.join(data_dir, meta_name)) as fp:
        meta = json.load(fp)
    images = np.stack([_read_png(os.path.join(data_dir, f["file_path"] + ".png")) for f in meta["frames"]])
    c2w = np.stack([np.asarray(f["transform_matrix"], dtype=np.float32) for f in meta["frames"]])
    w = images.shape[2]
    focal = 0.5 * w / math.tan(0.5 * float(meta["camera_angle_x"]))
    if dataset == "nerf_synthetic" and not multi_blocks:
        return images, c2w, focal
    if multi_blocks:
        labels = block_labels(c2w, num_blocks)
        out_i, out_c = [], []
        for b in sorted(set(int(v) for v in labels)):
            ids = _split_every_20(np.sort(np.nonzero(labels == b)[0]), split)
            out_i.append(images[ids])
            out_c.append(c2w[ids])
        return out_i, out_c, focal
    ids = _split_every_20(np.arange(images.shape[0]), split)
    return images[ids], c2w[ids], focal


class SubjectImages:
    """One scene (or one block of it) on the device: images uint8 [N,H,W,4], camtoworlds fp32 [N,4,4], K fp32 [3,3].
    sample(num_rays) draws random (image, x, y) pixels over all images and returns (Rays [num_rays,3], pixels fp32 [num_rays,3] over white),
    and with with_alpha=True the pixels' alpha [num_rays] as a third value."""

    def __init__(self, images: np.ndarray, camtoworlds: np.ndarray, focal: float, device, block_id: Optional[int] = None):
        self.device = torch.device(device)
        self.images = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
        self.camtoworlds = torch.from_numpy(np.ascontiguousarray(camtoworlds)).float().to(self.device)
        n, h, w = self.images.shape[:3]
        self.HEIGHT, self.WIDTH = h, w
        self.K = torch.tensor([[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1]], dtype=torch.float32, device=self.device)
        self.current_block = block_id

    def __len__(self):
        return self.images.shape[0]

    @staticmethod
    def load(dataset: str, root_dir: str, scene: str, split: str, device, multi_blocks: bool = False, num_blocks: int = 1) -> List["SubjectImages"]:
        """Every block of a scene's split (one entry without --multi_blocks)."""
        images, c2w, focal = load_renderings(dataset, root_dir, scene, split, multi_blocks, num_blocks)
        if multi_blocks:
            return [SubjectImages(i, c, focal, device, block_id=b) for b, (i, c) in enumerate(zip(images, c2w))]
        return [SubjectImages(images, c2w, focal, device)]

    def rays_of(self, img: torch.Tensor, x: torch.Tensor, y: torch.Tensor, with_alpha: bool = False):
        """Rays through pixel centres (x, y) of images img (render.pixel_rays' rule, OpenGL cameras) and their pixels over white; with_alpha:
        also the pixels' alpha channel in [0,1], fp32 [N], as a third value (the target of NGPTrainer's opacity loss)."""
        K = self.K
        c2w = self.camtoworlds[img]
        cam = torch.stack([(x.float() - K[0, 2] + 0.5) / K[0, 0], -(y.float() - K[1, 2] + 0.5) / K[1, 1], -torch.ones_like(x, dtype=torch.float32)], dim=-1)
        directions = (cam[:, None, :] * c2w[:, :3, :3]).sum(dim=-1)
        origins = c2w[:, :3, -1].contiguous()
        viewdirs = directions / torch.linalg.norm(directions, dim=-1, keepdim=True)
        rgba = self.images[img, y, x].float() / 255.0
        pixels = rgba[:, :3] * rgba[:, 3:4] + (1.0 - rgba[:, 3:4])
        if with_alpha:
            return Rays(origins, viewdirs.contiguous()), pixels, rgba[:, 3].contiguous()
        return Rays(origins, viewdirs.contiguous()), pixels

    def sample(self, num_rays: int, generator: Optional[torch.Generator] = None, with_alpha: bool = False):
        n = len(self)
        img = torch.randint(0, n, (num_rays,), device=self.device, generator=generator)
        x = torch.randint(0, self.WIDTH, (num_rays,), device=self.device, generator=generator)
        y = torch.randint(0, self.HEIGHT, (num_rays,), device=self.device, generator=generator)
        return self.rays_of(img, x, y, with_alpha) if with_alpha else self.rays_of(img, x, y)

    def view(self, i: int):
        """(Rays [H,W,3], pixels [H,W,3] over white) of image i, for validation."""
        h, w = self.HEIGHT, self.WIDTH
        y, x = torch.meshgrid(torch.arange(h, device=self.device), torch.arange(w, device=self.device), indexing="ij")
        img = torch.full_like(x.reshape(-1), i)
        rays, pixels = self.rays_of(img, x.reshape(-1), y.reshape(-1))
        return Rays(rays.origins.view(h, w, 3), rays.viewdirs.view(h, w, 3)), pixels.view(h, w, 3)
