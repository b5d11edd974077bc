"""CPU: the image-metrics rule.  The fp32 restatement (tests/image_metrics_restatement.py) reproduces what the reference's own
ssim() / compute_psnr returned for the committed inputs (tests/golden/image_metrics.npz, written by tools/make_image_metrics_golden.py); the fp64
restatement agrees with them within the bound the HIP kernel is held to; the closed forms hold; every seeded defect of the restatement breaks that
bound on at least one case of the list tests/test_hip_image_metrics.py runs; the metrics.json writer and the point-cloud selection on synthetic
tensors."""
import json
import math
import os

import numpy as np
import pytest
import torch

import image_metrics_restatement as IR
from dreg_nerf_amd import image_metrics as IM

ULP1 = 2.0 ** -23


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "image_metrics.npz"))


def test_golden_file_covers_the_case_list(golden):
    assert {k.split("/")[0] for k in golden.files} == set(IR.CASE_NAMES)
    for case in IR.CASES:
        pred, gt = IR.make_images(case)
        assert np.array_equal(golden[case[0] + "/pred"], pred.numpy()) and np.array_equal(golden[case[0] + "/gt"], gt.numpy()), case[0]
        assert golden[case[0] + "/ssim"].shape == (case[2],) and golden[case[0] + "/psnr"].shape == (case[2],)


@pytest.mark.parametrize("case", IR.CASES, ids=IR.CASE_NAMES)
def test_fp32_restatement_reproduces_the_reference(golden, case):
    """A few ulp: 4 ulp(1) on SSIM (values up to 1), 4 ulp(32) on PSNR (values in [32, 64) at most)."""
    pred, gt = torch.from_numpy(golden[case[0] + "/pred"]), torch.from_numpy(golden[case[0] + "/gt"])
    r32 = IR.run(pred, gt, torch.float32)
    assert r32["ssim"].dtype == torch.float32
    assert np.abs(r32["ssim"].numpy().astype(np.float64) - golden[case[0] + "/ssim"]).max() <= 4 * ULP1
    assert np.abs(r32["psnr"].numpy().astype(np.float64) - golden[case[0] + "/psnr"]).max() <= 4 * 2.0 ** -18


@pytest.mark.parametrize("case", IR.CASES, ids=IR.CASE_NAMES)
def test_fp64_restatement_agrees_with_the_reference_within_the_kernels_bound(golden, case):
    """The reference's fp32 values lie within max(4 E_ref, floor) of the fp64 restatement, E_ref being the fp32 restatement's own error: the kernel's
    bound before its caps.  With the caps (1e-5 on SSIM, 1e-3 dB) they do as well on every content but the constant pair, where fp32 filtering is
    6e-5 off in SSIM (the same rounding at every interior pixel, divided by C2)."""
    _, _, r64, _, bd = IR.reference(case)
    assert bd["ssim"] <= IR.SSIM_CAP and bd["psnr"] <= IR.PSNR_CAP and bd["ssim_map"] <= IR.MAP_CAP
    e_ssim = np.abs(r64["ssim"].numpy() - golden[case[0] + "/ssim"]).max()
    e_psnr = np.abs(r64["psnr"].numpy() - golden[case[0] + "/psnr"]).max()
    assert e_ssim <= bd["uncapped"][1] and e_psnr <= bd["uncapped"][2]
    if case[1] != "constant":
        assert e_ssim <= bd["ssim"] and e_psnr <= bd["psnr"]


def test_taps_are_the_references_window():
    g = IR.taps()
    assert g.dtype == torch.float32 and g.shape == (11,) and torch.equal(g, g.flip(0)) and abs(float(g.sum()) - 1.0) <= 2 * ULP1
    assert torch.equal(IM.gaussian_taps(), g)
    assert float(g[5]) == pytest.approx(1.0 / sum(math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)), rel=1e-6)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_identical_images_give_one_and_sixty(dtype):
    for case in IR.CASES:
        if case[1] != "identical":
            continue
        pred, gt = IR.make_images(case)
        r = IR.run(pred, gt, dtype)
        assert torch.equal(r["ssim_map"], torch.ones_like(r["ssim_map"])) and torch.equal(r["mse"], torch.zeros_like(r["mse"]))
        assert (r["psnr"].double() - 60.0).abs().max().item() <= (1e-12 if dtype == torch.float64 else 2.0 ** -18)


def test_constant_pair_closed_form_in_the_interior():
    """A pixel more than 5 from every border sees the whole window over constants a, b: mu = a, b exactly (the taps sum to 1), sigma = 0, so
    ssim = (2ab + C1) / (a^2 + b^2 + C1)."""
    case = IR.CASES[IR.CASE_NAMES.index("constant_32x32")]
    _, _, r64, _, _ = IR.reference(case)
    a, b = (float(torch.tensor(v, dtype=torch.float32)) for v in IR.CONSTANT_PAIR)
    s = float(IR.taps().double().sum()) ** 2                 # the fp32 taps sum to 1 within an ulp; the closed form with that sum, exactly
    ma, mb = a * s, b * s
    want = (2 * ma * mb + IR.C1) * (2 * (a * b * s - ma * mb) + IR.C2) / ((ma * ma + mb * mb + IR.C1) * (a * a * s - ma * ma + b * b * s - mb * mb + IR.C2))
    inner = r64["ssim_map"][:, 5:-5, 5:-5]
    assert inner.numel() > 0 and (inner - want).abs().max().item() < 1e-12
    # with taps summing to exactly 1 this is (2ab + C1) / (a^2 + b^2 + C1); their fp32 sum is off by up to 2 ulp(1), which sigma = a^2 s (1 - s) carries into the C2 factors
    assert abs(s - 1.0) <= 4 * ULP1 and abs(want - (2 * a * b + IR.C1) / (a * a + b * b + IR.C1)) < IR.MAP_FLOOR
    # the border is NOT renormalised: a corner pixel sees about a quarter of the window's mass
    assert float(r64["ssim_map"][0, 0, 0, 0]) != pytest.approx(want, abs=1e-3)


def test_one_by_one_image_by_hand():
    """H = W = 1: only the centre tap meets the pixel: mu = w x, E[x^2] = w x^2 with w = g[5]^2."""
    case = IR.CASES[IR.CASE_NAMES.index("noise_1x1")]
    pred, gt, r64, _, _ = IR.reference(case)
    x, y, w = float(pred.reshape(-1)[0]), float(gt.reshape(-1)[0]), float(IR.taps()[5].double()) ** 2
    m1, m2 = w * x, w * y
    want = (2 * m1 * m2 + IR.C1) * (2 * (w * x * y - m1 * m2) + IR.C2) / ((m1 * m1 + m2 * m2 + IR.C1) * (w * x * x - m1 * m1 + w * y * y - m2 * m2 + IR.C2))
    assert float(r64["ssim"][0]) == pytest.approx(want, abs=1e-14)
    assert float(r64["mse"][0]) == pytest.approx((x - y) ** 2, abs=1e-15)
    assert float(r64["psnr"][0]) == pytest.approx(-10 * math.log10((x - y) ** 2 + 1e-6), abs=1e-10)


@pytest.mark.parametrize("defect", IR.DEFECTS)
def test_every_seeded_defect_is_caught(defect):
    """A kernel with this one defect would fail tests/test_hip_image_metrics.py: on at least one case of its list an error exceeds that case's bound."""
    caught = []
    for case in IR.CASES:
        pred, gt, r64, _, bd = IR.reference(case)
        bad = IR.run(pred, gt, torch.float64, **{defect: True})
        e_map, e_ssim, e_psnr = IR.errors(bad, r64)
        over = lambda e, b: not (e <= b)                     # (inf and nan count as caught)
        if over(e_map, bd["ssim_map"]) or over(e_ssim, bd["ssim"]) or over(e_psnr, bd["psnr"]):
            caught.append(case[0])
    assert caught, f"no case of the list notices {defect}: extend the list"


def test_metrics_json_schema(tmp_path):
    path = tmp_path / "metrics.json"
    d = IM.write_metrics_json(str(path), "chair", [30.0, 32.0, 31.0], [0.9, 0.95, 0.85])
    back = json.load(open(path))
    assert back == d and set(back) == {"chair"}
    assert set(back["chair"]) == {"0", "1", "2", "psnr", "ssim"} and "lpips" not in back["chair"]
    assert back["chair"]["1"] == {"psnr": 32.0, "ssim": 0.95}
    assert back["chair"]["psnr"] == pytest.approx(31.0) and back["chair"]["ssim"] == pytest.approx(0.9)
    with pytest.raises(ValueError):
        IM.metrics_dict("chair", [], [])


def test_point_cloud_selection():
    g = torch.Generator().manual_seed(0)
    views = []
    for cam in range(2):
        o = torch.randn(3, generator=g).expand(4, 5, 3)
        d = torch.nn.functional.normalize(torch.randn(4, 5, 3, generator=g), dim=-1)
        z = torch.rand(4, 5, 1, generator=g) * 8.0
        z[0, 0, 0], z[0, 1, 0], z[0, 2, 0] = 2.0, 6.0, 0.0     # both ends of the range are kept; a missed ray (depth 0) is not
        views.append((o, d, z, torch.rand(4, 5, 3, generator=g)))
    pts, cols = IM.point_cloud_from_views(views)
    want_p, want_c = [], []
    for o, d, z, rgb in views:                                 # camera, then pixel order
        for i in range(20):
            zz = float(z.reshape(-1)[i])
            if 2.0 <= zz <= 6.0:
                want_p.append(o.reshape(-1, 3)[i] + d.reshape(-1, 3)[i] * zz)
                want_c.append(rgb.reshape(-1, 3)[i])
    assert 0 < len(want_p) < 40 and pts.shape == (len(want_p), 3) and cols.shape == pts.shape
    assert torch.allclose(pts, torch.stack(want_p), atol=1e-6) and torch.equal(cols, torch.stack(want_c))
    p2, _ = IM.select_depth_points(*views[0], min_depth=0.0, max_depth=100.0)
    assert p2.shape[0] == 20


def test_image_metrics_refuses_gradients_and_host_tensors():
    x = torch.rand(4, 4, 3)
    with pytest.raises(RuntimeError, match="no backward"):
        IM.image_metrics(x.clone().requires_grad_(), x)
    with pytest.raises(ValueError):
        IM.image_metrics(x, x)                                 # no CPU path
    with pytest.raises(ValueError):
        IM.image_metrics(x, x[:3])


def test_evaluator_finds_the_trainers_checkpoints(tmp_path):
    """eval_ngp_nerf.py --eval_images: --ckpt_path, else <root>/out/<expname>/model.pth, else block_k/model.pth of every block_* directory in block order."""
    import importlib.util
    from types import SimpleNamespace
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_eval_ngp_nerf", os.path.join(root, "eval_ngp_nerf.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    base = tmp_path / "out" / "exp"
    for k in (0, 1, 10, 2):
        (base / f"block_{k}").mkdir(parents=True)
    cfg = SimpleNamespace(ckpt_path="", root_dir=str(tmp_path), expname="exp", multi_blocks=False)
    assert E.block_checkpoints(cfg) == ([(None, str(base / "model.pth"))], 1)
    cfg.multi_blocks = True
    ckpts, n = E.block_checkpoints(cfg)
    assert n == 4 and [k for k, _ in ckpts] == [0, 1, 2, 10] and ckpts[3][1] == str(base / "block_10" / "model.pth")
    cfg.multi_blocks, cfg.ckpt_path = False, "/somewhere/model.pth"
    assert E.block_checkpoints(cfg) == ([(None, "/somewhere/model.pth")], 1)
    cfg.expname, cfg.ckpt_path, cfg.multi_blocks = "none", "", True
    with pytest.raises(FileNotFoundError):
        E.block_checkpoints(cfg)
