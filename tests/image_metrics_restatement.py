"""CPU restatement of the image-metrics rule (the reference's conerf/loss/ssim_torch.py and compute_psnr) in torch, in fp64 and in
fp32, both returning the SSIM map.  The fp32 form performs the reference's operations (grouped 11x11 conv2d with the fp32 outer-product window) and
reproduces the golden values of tests/golden/image_metrics.npz; the fp64 form is what the HIP kernel is measured against, and the fp32 form's own
error against it sizes the kernel's bound (`bounds`).  Through its defect switches tests/test_image_metrics_host.py shows that the case list of
tests/test_hip_image_metrics.py notices each of the ways a tiled, haloed kernel goes wrong.

Images are channel-last [N,H,W,C] like the kernel's."""
import math

import numpy as np
import torch
import torch.nn.functional as F

WINDOW, PAD, TILE = 11, 5, 32
C1, C2 = 0.01 ** 2, 0.03 ** 2
EPS = 1e-6

DEFECTS = ("window_shifted", "halo_zero_at_tile_edge", "border_renormalised", "reflect_padding", "sigma_one", "c1_c2_swapped", "interior_mean",
           "psnr_no_eps")

# (name, content, N, H, W, C): every size at which a 32x32-tiled kernel with a 5-pixel halo takes another path — smaller than the window, exactly
# one tile, one past a tile, ragged in both axes — with N in {1, 3} and C in {1, 3, 4} spread over them, and each content at several sizes.
CASES = [
    ("noise_1x1", "noise", 1, 1, 1, 1),
    ("identical_1x1", "identical", 1, 1, 1, 4),
    ("noise_1x40", "noise", 3, 1, 40, 3),
    ("noise_7x9", "noise", 1, 7, 9, 4),
    ("constant_7x9", "constant", 3, 7, 9, 3),
    ("patch_11x11", "patch", 1, 11, 11, 3),
    ("sinus_11x11", "sinus", 3, 11, 11, 4),
    ("noise_32x32", "noise", 3, 32, 32, 1),
    ("constant_32x32", "constant", 1, 32, 32, 4),
    ("patch_33x47", "patch", 1, 33, 47, 3),
    ("identical_33x47", "identical", 1, 33, 47, 3),
    ("sinus_33x47", "sinus", 3, 33, 47, 1),
    ("noise_33x47", "noise", 1, 33, 47, 4),
    ("sinus_31x96", "sinus", 1, 31, 96, 4),
    ("patch_31x96", "patch", 1, 31, 96, 3),
    ("noise_64x65", "noise", 1, 64, 65, 3),
    ("patch_64x65", "patch", 3, 64, 65, 1),
]
CASE_NAMES = [c[0] for c in CASES]
CONSTANT_PAIR = (0.3, 0.7)
BIG_CASE = ("noise_800x800", "noise", 2, 800, 800, 3)        # the evaluator's size: grid and partial-sum count (GPU test only, not in the golden file)


def make_images(case):
    """(pred, gt) fp32 [N,H,W,C] of a case, deterministic."""
    name, content, n, h, w, c = case
    g = torch.Generator().manual_seed(1000 + sum(ord(ch) for ch in name))
    shape = (n, h, w, c)
    if content == "noise":                                   # uniform noise, 0.1 Gaussian error (values leave [0,1]: the uint8 clamp is exercised)
        gt = torch.rand(shape, generator=g)
        pred = gt + 0.1 * torch.randn(shape, generator=g)
    elif content == "patch":                                 # the renderer's regime: white background, a textured patch, error on the patch only
        gt = torch.ones(shape)
        y0, y1, x0, x1 = h // 4, max(h // 4 + 1, 3 * h // 4), w // 4, max(w // 4 + 1, 3 * w // 4)
        gt[:, y0:y1, x0:x1] = torch.rand((n, y1 - y0, x1 - x0, c), generator=g)
        pred = gt.clone()
        pred[:, y0:y1, x0:x1] += 0.05 * torch.randn((n, y1 - y0, x1 - x0, c), generator=g)
        pred = pred.clamp(0.0, 1.0)
    elif content == "sinus":                                 # smooth, 0.01 error
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        ph = torch.arange(n * c, dtype=torch.float32).reshape(n, 1, 1, c)
        gt = 0.5 + 0.4 * torch.sin(2 * math.pi * (3 * xx / max(w, 1) + 2 * yy / max(h, 1))[None, :, :, None] + ph)
        pred = gt + 0.01 * torch.randn(shape, generator=g)
    elif content == "identical":
        gt = torch.rand(shape, generator=g)
        pred = gt.clone()
    elif content == "constant":
        pred, gt = torch.full(shape, CONSTANT_PAIR[0]), torch.full(shape, CONSTANT_PAIR[1])
    else:
        raise ValueError(content)
    return pred.float().contiguous(), gt.float().contiguous()


def taps(sigma=1.5):
    """ssim_torch.gaussian: Python floats -> fp32 -> divided by their fp32 sum."""
    g = torch.tensor([math.exp(-(x - WINDOW // 2) ** 2 / float(2 * sigma ** 2)) for x in range(WINDOW)], dtype=torch.float32)
    return g / g.sum()


def _window(c, dtype, sigma):
    g = taps(sigma)
    if dtype == torch.float32:
        w2 = g.unsqueeze(1).mm(g.unsqueeze(1).t())            # the reference's fp32 product
    else:
        w2 = torch.outer(g.double(), g.double())              # the fp32 taps, their products exact
    return w2.to(dtype)[None, None].expand(c, 1, WINDOW, WINDOW).contiguous()


def run(pred, gt, dtype=torch.float64, separable=False, **defects):
    """pred, gt [N,H,W,C] -> dict(ssim_map [N,H,W,C], ssim [N], mse [N], psnr [N]) in `dtype`.  `defects`: any of DEFECTS=True seeds that one defect.
    separable (fp64 only, no defects): the window applied as a row pass and a column pass — the same sums up to fp64 rounding at a fifth of the
    work, for the one large case."""
    assert not separable or (dtype == torch.float64 and not defects)
    for name in defects:
        assert name in DEFECTS, name
    df = lambda name: bool(defects.get(name, False))
    x = pred.permute(0, 3, 1, 2).to(dtype)                    # img1 / img2 of the reference, [N,C,H,W]
    y = gt.permute(0, 3, 1, 2).to(dtype)
    n, c, h, w = x.shape
    window = _window(c, dtype, 1.0 if df("sigma_one") else 1.5)

    def conv(img):
        if separable:
            g = taps().double()[None, None].expand(c, 1, 1, WINDOW).contiguous()
            return F.conv2d(F.conv2d(img, g, padding=(0, PAD), groups=c), g.transpose(2, 3).contiguous(), padding=(PAD, 0), groups=c)
        if df("window_shifted"):
            return F.conv2d(F.pad(img, (PAD + 1, PAD - 1, PAD + 1, PAD - 1)), window, groups=c)
        if df("reflect_padding") and min(h, w) > PAD:
            return F.conv2d(F.pad(img, (PAD,) * 4, mode="reflect"), window, groups=c)
        return F.conv2d(img, window, padding=PAD, groups=c)

    def filt(img):
        if df("halo_zero_at_tile_edge"):                      # every 32x32 tile filtered as if it were the whole image
            out = torch.empty_like(img)
            for ty in range(0, h, TILE):
                for tx in range(0, w, TILE):
                    out[:, :, ty:ty + TILE, tx:tx + TILE] = conv(img[:, :, ty:ty + TILE, tx:tx + TILE])
            return out
        out = conv(img)
        if df("border_renormalised"):
            out = out / F.conv2d(torch.ones_like(img), window, padding=PAD, groups=c)
        return out

    mu1, mu2 = filt(x), filt(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = filt(x * x) - mu1_sq
    sigma2_sq = filt(y * y) - mu2_sq
    sigma12 = filt(x * y) - mu1_mu2
    c1, c2 = (C2, C1) if df("c1_c2_swapped") else (C1, C2)
    smap = ((2 * mu1_mu2 + c1) * (2 * sigma12 + c2)) / ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2))
    if df("interior_mean") and h > 2 * PAD and w > 2 * PAD:
        ssim = smap[:, :, PAD:h - PAD, PAD:w - PAD].reshape(n, -1).mean(dim=1)
    else:
        ssim = smap.reshape(n, -1).mean(dim=1)
    mse = ((x - y) ** 2).reshape(n, -1).mean(dim=1)
    psnr = -10.0 * torch.log(mse + (0.0 if df("psnr_no_eps") else EPS)) / np.log(10.0)
    return {"ssim_map": smap.permute(0, 2, 3, 1).contiguous(), "ssim": ssim, "mse": mse, "psnr": psnr}


# ---------------------------------------------------------------------------------------------------------------- the kernel's bounds
# Per map pixel.  The two factors that carry C2, (2 sigma12 + C2) and (sigma1^2 + sigma2^2 + C2), are built from differences E[.] - mu^2 of fp32
# numbers of size up to 1.  Each side of such a difference ends in a rounding of half an ulp(1) at best (the last accumulate of the filter, the
# product mu * mu), so a sigma term computed by two correct fp32 programs with different summation orders differs by up to ~2 ulp(1), and the
# numerator and denominator factors together by ~4 ulp(1) = 4 * 2^-23.  Where the image is flat (sigma ~ 0: the white background of a render) the
# factors are ~C2 and the map value ~1, so that absolute difference becomes a RELATIVE one of 4 ulp(1) / C2 = 5.3e-4 in the map.  No fp32 program
# can promise less; four times the torch restatement's measured error is allowed on top where that is larger (a separable, tiled filter sums in
# another order), and the issue's cap of 4e-3 holds in every case.
ULP1 = 2.0 ** -23
MAP_FLOOR = 4 * ULP1 / C2
MAP_CAP = 4e-3
# Per-image SSIM: the mean of M = H W C map values whose errors are roundings of both signs, each within MAP_FLOOR: their mean moves by
# MAP_FLOOR / sqrt(M) (random signs), plus the rounding of the fp32 result itself, half an ulp(1) = 2^-24.  Cap: 1e-5.  (On the constant pair the
# roundings are NOT of both signs — every interior pixel repeats the same one — and the fp32 restatement, like the reference, is 6e-5 off there: the
# cap is then the kernel's bound, which is why the kernel filters in fp64.  `uncapped` is what the reference's own numbers are held to on the host.)
SSIM_CAP = 1e-5
# PSNR: (x - y)^2 carries two fp32 roundings (2^-24 relative each), so mse is good to ~2^-23 relative and psnr = -10 log10(mse + eps) to
# 10 / ln 10 * 2^-23 = 5e-7 dB; the fp32 result itself (values in [32, 64): identical images sit at 60) rounds by half an ulp = 2^-19 = 1.9e-6 dB.
# Floor: twice that rounding, 2^-18 dB.  Cap: 1e-3 dB.
PSNR_FLOOR = 2.0 ** -18
PSNR_CAP = 1e-3


def ssim_floor(numel_per_image):
    return MAP_FLOOR / math.sqrt(numel_per_image) + 2.0 ** -24


def bounds(ref64, ref32):
    """The kernel's allowed error against ref64 for one case: max(4 E_ref, floor) capped, E_ref = the fp32 torch restatement's error against fp64.
    -> dict(ssim_map, ssim, psnr, e_ref=(map, ssim, psnr))."""
    e_map = (ref32["ssim_map"].double() - ref64["ssim_map"]).abs().max().item()
    e_ssim = (ref32["ssim"].double() - ref64["ssim"]).abs().max().item()
    e_psnr = (ref32["psnr"].double() - ref64["psnr"]).abs().max().item()
    m = ref64["ssim_map"][0].numel()
    uncapped = (max(4 * e_map, MAP_FLOOR), max(4 * e_ssim, ssim_floor(m)), max(4 * e_psnr, PSNR_FLOOR))
    return {"ssim_map": min(uncapped[0], MAP_CAP), "ssim": min(uncapped[1], SSIM_CAP), "psnr": min(uncapped[2], PSNR_CAP),
            "e_ref": (e_map, e_ssim, e_psnr), "uncapped": uncapped}


def errors(got, ref64):
    """(map, ssim, psnr) max abs errors of a result dict against the fp64 restatement (the map is optional)."""
    e_map = (got["ssim_map"].double() - ref64["ssim_map"]).abs().max().item() if got.get("ssim_map") is not None else 0.0
    return (e_map, (got["ssim"].double() - ref64["ssim"]).abs().max().item(), (got["psnr"].double() - ref64["psnr"]).abs().max().item())


_cache = {}


def reference(case):
    """(pred, gt, ref64, ref32, bounds) of a case, computed once and shared; callers must not modify it."""
    key = case[0]
    if key not in _cache:
        pred, gt = make_images(case)
        if case is BIG_CASE:
            # the large case would spend its seconds in the fp32 restatement's 121-tap convolution: it gets the floors alone (never wider than
            # max(4 E_ref, floor)) against a separable fp64 restatement, and no fp32 one
            r64, r32 = run(pred, gt, torch.float64, separable=True), None
            bd = {"ssim_map": MAP_FLOOR, "ssim": min(ssim_floor(r64["ssim_map"][0].numel()), SSIM_CAP), "psnr": PSNR_FLOOR, "e_ref": None}
        else:
            r64, r32 = run(pred, gt, torch.float64), run(pred, gt, torch.float32)
            bd = bounds(r64, r32)
        _cache[key] = (pred, gt, r64, r32, bd)
    return _cache[key]
