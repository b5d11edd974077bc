"""GPU: the differentiable pose — the weighted Kabsch backward (csrc/pointset.hip kabsch_bwd_kernel / kabsch_pairs_bwd_kernel) against the
reference's own autograd (tests/golden/kabsch_grad.npz, tools/make_golden_pose_grad.py), at repeated singular values against central differences of
the fp64 oracle, pair form against dense form; NeRFRegTr(differentiable_pose=True) against the reference network (tests/golden/pose_grad32.npz); the
opt-in pose loss of TrainStep."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dreg_nerf_amd import attn_ops as A, losses as LS, params, pointset_exec, synth  # noqa: E402
from dreg_nerf_amd import lib as L  # noqa: E402
from dreg_nerf_amd.regtr import NeRFRegTr  # noqa: E402
from dreg_nerf_amd.train_step import TrainStep  # noqa: E402
from oracle import regtr_oracle as O  # noqa: E402

DEV = "cuda:0"
CASES = ["n3", "n17", "n255", "n256", "n257", "n3000", "zeros", "reflection", "small_sum", "planar"]


def _rel(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))


def _dense_grads(a, b, w, g):
    a, b, w = (t.to(DEV).requires_grad_(True) for t in (a, b, w))
    T = A.weighted_kabsch_grad(a, b, w)
    T.backward(g.to(DEV))
    return T.detach().cpu(), a.grad.cpu(), b.grad.cpu(), w.grad.cpu()


@pytest.mark.parametrize("case", CASES)
def test_dense_backward_matches_reference_autograd(golden_dir, case):
    z = np.load(os.path.join(golden_dir, "kabsch_grad.npz"))
    a, b, w, g = (torch.from_numpy(z[f"{case}/{k}"]) for k in ("a", "b", "w", "g_out"))
    T, ga, gb, gw = _dense_grads(a[None], b[None], w[None], g[None])
    np.testing.assert_allclose(T[0].numpy(), z[f"{case}/pose"], atol=1e-4 if case == "planar" else 1e-5)
    tol = 1e-3 if case == "planar" else 1e-5
    for got, k in ((ga[0], "g_a"), (gb[0], "g_b"), (gw[0], "g_w")):
        assert torch.isfinite(got).all()
        err = _rel(got.numpy(), z[f"{case}/{k}"])
        assert err <= tol, (case, k, err)


def test_repeated_singular_values_finite_and_match_central_differences():
    """An isotropic xy spread (points evenly on a circle, equal weights): s1 = s2 (to fp32 rounding), where torch's SVD backward divides by s1^2 - s2^2 = 0.  The kernel's
    denominators are s~_i + s~_j: the gradient is finite and equals central differences of the fp64 oracle forward."""
    n = 64
    th = torch.arange(n, dtype=torch.float64) * (2 * np.pi / n)
    a = torch.stack([torch.cos(th) * 1.5, torch.sin(th) * 1.5, 0.2 * torch.cos(3 * th + 0.4)], 1).float()
    q = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64))[0]
    q = q if torch.det(q) > 0 else -q
    # not a rigid copy (an exact fit has a zero weight gradient): scaled isotropically in xy, so H = diag(c s, c s, c_z s_z) q^T keeps s1 = s2
    b = ((a.double() * torch.tensor([1.3, 1.3, 0.7], dtype=torch.float64)) @ q.T + torch.tensor([0.3, -0.1, 0.5], dtype=torch.float64)).float()
    w = torch.full((n,), 0.5)
    s = torch.linalg.svdvals((a.double() - a.double().mean(0)).T @ (b.double() - b.double().mean(0)))
    assert float((s[0] - s[1]).abs() / s[0]) < 1e-6            # repeated
    g = torch.randn(3, 4, generator=torch.Generator().manual_seed(5))
    _, ga, gb, gw = _dense_grads(a[None], b[None], w[None], g[None])
    for t in (ga, gb, gw):
        assert torch.isfinite(t).all()
    f = lambda a_, b_, w_: float((O.weighted_kabsch(a_, b_, w_) * g.double()).sum())
    a64, b64, w64 = a.double(), b.double(), w.double()
    gen = torch.Generator().manual_seed(6)
    h = 1e-6
    for which, grad in (("a", ga[0]), ("b", gb[0]), ("w", gw[0])):
        for _ in range(3):
            v = torch.randn((n, 3) if which != "w" else (n,), generator=gen, dtype=torch.float64)
            args_p, args_m = [a64, b64, w64], [a64, b64, w64]
            i = "abw".index(which)
            args_p[i], args_m[i] = args_p[i] + h * v, args_m[i] - h * v
            fd = (f(*args_p) - f(*args_m)) / (2 * h)
            an = float((grad.double() * v).sum())
            assert abs(an - fd) <= 1e-4 * max(abs(fd), float(grad.double().norm() * v.norm())), (which, an, fd)


def _pairs_case(seed, segs, extra=0):
    g = torch.Generator().manual_seed(seed)
    tab = A.ProblemTable(segs, torch.device(DEV))
    R = tab.R + extra                                                       # rows past tab.R: covered by no problem
    xyz = (torch.rand(R, 3, generator=g) - 0.5) * 1.6
    corr = xyz[None] + 0.1 * torch.randn(6, R, 3, generator=g)
    ov = torch.sigmoid(torch.randn(6, R, 1, generator=g))
    gout = torch.randn(len(segs), 6, 3, 4, generator=g)
    return tab, xyz.to(DEV), corr.to(DEV), ov.to(DEV), gout.to(DEV)


def test_pairs_backward_equals_dense_form_bit_for_bit():
    segs = [(310, 277), (150, 401), (64, 64), (3, 5)]
    tab, xyz, corr, ov, gout = _pairs_case(7, segs)
    c, o = corr.clone().requires_grad_(True), ov.clone().requires_grad_(True)
    T = A.weighted_kabsch_pairs_grad(xyz, c, o, tab)
    assert torch.equal(T.detach(), A.weighted_kabsch_pairs(xyz, corr, ov, tab))       # the forward launch is today's
    T.backward(gout)
    assert c.grad.shape == corr.shape and o.grad.shape == ov.shape                      # ov's gradient in the shape it came in ([L,R,1])
    for p, (s0, ns, t0, nt) in enumerate(tab.segs):
        a = torch.cat([xyz[s0:s0 + ns].expand(6, -1, -1), corr[:, t0:t0 + nt]], dim=1).contiguous()
        b = torch.cat([corr[:, s0:s0 + ns], xyz[t0:t0 + nt].expand(6, -1, -1)], dim=1).contiguous()
        w = torch.cat([ov[:, s0:s0 + ns, 0], ov[:, t0:t0 + nt, 0]], dim=1).contiguous()
        _, ga, gb, gw = _dense_grads(a.cpu(), b.cpu(), w.cpu(), gout[p].cpu())
        gc, go = c.grad.cpu(), o.grad.cpu()[..., 0]
        assert torch.equal(gc[:, s0:s0 + ns], gb[:, :ns]), p          # source rows: corr is b
        assert torch.equal(gc[:, t0:t0 + nt], ga[:, ns:]), p          # target rows: corr is a
        assert torch.equal(go[:, s0:s0 + ns], gw[:, :ns]) and torch.equal(go[:, t0:t0 + nt], gw[:, ns:]), p
    # every layer's correspondences receive a gradient
    assert all(float(c.grad[l].abs().sum()) > 0 for l in range(6))
    # [L,R] form of ov
    o2 = ov[..., 0].clone().requires_grad_(True)
    A.weighted_kabsch_pairs_grad(xyz, corr, o2, tab).backward(gout)
    assert o2.grad.shape == (6, tab.R) and torch.equal(o2.grad, o.grad[..., 0])


def test_pairs_backward_writes_zeros_on_uncovered_rows_and_is_deterministic():
    segs = [(120, 77), (50, 91)]
    tab, xyz, corr, ov, gout = _pairs_case(8, segs, extra=300)
    R = xyz.shape[0]
    ov2 = ov[..., 0].contiguous()
    outs = []
    for _ in range(2):
        gc = torch.full((6, R, 3), float("nan"), device=DEV)
        go = torch.full((6, R), float("nan"), device=DEV)
        L.check(L.load().dreg_weighted_kabsch_pairs_bwd(L.ptr(xyz), L.ptr(corr), L.ptr(ov2), L.ptr(tab.pair_probs), L.ptr(gout), L.ptr(gc), L.ptr(go),
                                                        len(segs), 6, R, 1e-6, L.stream()), "dreg_weighted_kabsch_pairs_bwd")
        outs.append((gc.cpu(), go.cpu()))
    gc, go = outs[0]
    assert torch.isfinite(gc).all() and torch.isfinite(go).all()
    assert float(gc[:, tab.R:].abs().max()) == 0.0 and float(go[:, tab.R:].abs().max()) == 0.0
    assert float(gc[:, :tab.R].abs().sum()) > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # null outputs are skipped
    L.check(L.load().dreg_weighted_kabsch_pairs_bwd(L.ptr(xyz), L.ptr(corr), L.ptr(ov2), L.ptr(tab.pair_probs), L.ptr(gout), None, L.ptr(go), len(segs), 6,
                                                    R, 1e-6, L.stream()), "dreg_weighted_kabsch_pairs_bwd")
    assert torch.equal(go.cpu(), outs[0][1])
    # dense form: two calls bit-identical
    z = [_dense_grads(corr[:, :200].cpu(), xyz[:200].expand(6, -1, -1).cpu(), ov2[:, :200].cpu(), gout[0].cpu()) for _ in range(2)]
    assert all(torch.equal(x, y) for x, y in zip(z[0], z[1]))


# ---------------------------------------------------------------------------------------------------------------- model
GROUPS = {"transformer": "transformer_encoder.", "decoder": "correspondence_decoder."}


def _pose_model(precision, differentiable=True):
    """pose_grad32.npz's setting: params.synth_state_dict(0), eval-mode BatchNorm, the feature network frozen; preallocated gradient buffers (what
    FlatAdamW gives the native point-set executor)."""
    m = NeRFRegTr(precision=precision, differentiable_pose=differentiable)
    m.load_state_dict(params.synth_state_dict(0), strict=True)
    m = m.cuda().eval()
    for k, p in m.named_parameters():
        p.requires_grad_(k.startswith(tuple(GROUPS.values())))
        p.grad = torch.zeros_like(p) if p.requires_grad else None
    return m


def _pose_loss_of(pred, data):
    return _ref_pose_loss(pred["pose"], pred["src_kp"][0], data["pose"][0].cuda())


def _ref_pose_loss(pose, kp, pose_gt):
    """An independent torch evaluation of the pose loss of one pair: poses [nl,1,3,4] or [nl,3,4], source key points [N,3], true pose [4,4]."""
    pose = pose.reshape(-1, 3, 4)
    moved = kp @ pose[:, :, :3].transpose(-1, -2) + pose[:, None, :, 3]
    target = kp @ pose_gt[:3, :3].T + pose_gt[:3, 3]
    return (moved - target).abs().sum(-1).mean(-1).mean()


def _model_grads(precision):
    m = _pose_model(precision)
    data = synth.shell_pair(32, 1, 2, pose=synth.fixed_pose())
    pred = m({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()})
    assert pred["pose"].requires_grad
    loss = _pose_loss_of(pred, data)
    loss.backward()
    torch.cuda.synchronize()
    return m, float(loss), dict(m.named_parameters())


def test_model_fp32_pose_gradient_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "pose_grad32.npz"))
    m, loss, named = _model_grads("fp32")
    np.testing.assert_allclose(loss, float(g["loss"]), rtol=1e-4)
    for name, pref in GROUPS.items():
        sq = sum(float(p.grad.double().pow(2).sum()) for k, p in named.items() if k.startswith(pref) and p.grad is not None)
        np.testing.assert_allclose(sq ** 0.5, float(g["gnorm64_" + name]), rtol=2e-2)
    # every decoder layer's parameters receive the pose loss's gradient
    for l in range(6):
        assert float(named[f"transformer_encoder.layers.{l}.linear2.weight"].grad.abs().sum()) > 0
    for key in g.files:
        if key.startswith("gidx/"):
            k = key[5:]
            got = named[k].grad.flatten().cpu()[g[key]].double().numpy()
            ref32, ref64 = g["gval/" + k].astype(np.float64), g["gval64/" + k]
            scale = np.linalg.norm(ref64)
            err_ref, err_got = np.linalg.norm(ref32 - ref64) / scale, np.linalg.norm(got - ref64) / scale
            assert err_got <= max(4 * err_ref, 2e-3), (k, err_got, err_ref)


def test_model_bf16_executor_pose_gradient_close_to_fp32(monkeypatch):
    calls = []
    orig = pointset_exec.PointSetExecutor.backward

    def spy(self, *a, **kw):
        calls.append(kw.get("last_only", False))
        return orig(self, *a, **kw)
    monkeypatch.setattr(pointset_exec.PointSetExecutor, "backward", spy)
    _, _, n32 = _model_grads("fp32")
    assert not calls                                   # fp32: the per-op path
    _, _, n16 = _model_grads("bf16")
    assert calls == [False]                            # bf16: the native executor, its full (all six layers) backward
    for name, pref in GROUPS.items():
        a = sum(float(p.grad.double().pow(2).sum()) for k, p in n16.items() if k.startswith(pref) and p.grad is not None) ** 0.5
        b = sum(float(p.grad.double().pow(2).sum()) for k, p in n32.items() if k.startswith(pref) and p.grad is not None) ** 0.5
        assert abs(a - b) <= 5e-2 * b, (name, a, b)
    for k in ("transformer_encoder.layers.0.self_attn.in_proj_weight", "transformer_encoder.layers.5.linear2.weight",
              "correspondence_decoder.q_proj.weight", "correspondence_decoder.conf_logits_decoder.weight"):
        x, y = n16[k].grad.double().flatten().cpu(), n32[k].grad.double().flatten().cpu()
        cos = float(x @ y / (x.norm() * y.norm()))
        assert cos >= 0.99, (k, cos)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_default_off_pose_detached_same_value(precision):
    data = synth.shell_pair(32, 1, 2, pose=synth.fixed_pose())
    poses = {}
    for flag in (False, True):
        m = _pose_model(precision, flag)
        assert m.differentiable_pose is flag
        pred = m({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()})
        assert pred["pose"].requires_grad is flag
        poses[flag] = pred["pose"].detach().cpu()
        with torch.no_grad():
            assert m({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in data.items()})["pose"].requires_grad is False
    assert torch.equal(poses[False], poses[True])
    assert NeRFRegTr().differentiable_pose is False


# ---------------------------------------------------------------------------------------------------------------- training step
def _steps(n, seed_w=5, **kw):
    m = NeRFRegTr(precision="bf16")
    m.load_state_dict(params.synth_state_dict(0), strict=True)
    m = m.cuda().train()
    ts = TrainStep(m, **kw)
    with torch.no_grad():
        ts.feature_loss.W.copy_((0.1 * torch.randn(256, 256, generator=torch.Generator().manual_seed(seed_w))).cuda())
    outs = []
    for i in range(n):
        data = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synth.shell_pair(64, 1 + i, 2 + i, pose=synth.fixed_pose()).items()}
        outs.append((ts.step([data]), data))
    torch.cuda.synchronize()
    return m, ts, outs


def test_train_step_weight_zero_is_unchanged():
    m0, ts0, o0 = _steps(3)
    m1, ts1, o1 = _steps(3, pose_loss_weight=0.0)
    for (k, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p, q), k
    assert set(o0[-1][0]["losses"]) == set(o1[-1][0]["losses"]) and "pose" not in o1[-1][0]["losses"]


@pytest.mark.parametrize("fused", [True, False])
def test_train_step_pose_loss_value_and_total(monkeypatch, fused):
    calls = []
    orig = pointset_exec.PointSetExecutor.backward

    def spy(self, *a, **kw):
        calls.append(kw.get("last_only", False))
        return orig(self, *a, **kw)
    monkeypatch.setattr(pointset_exec.PointSetExecutor, "backward", spy)
    w = 0.25
    for layers in ("last", "all"):
        calls.clear()
        m, ts, outs = _steps(1, pose_loss_weight=w, pose_loss_layers=layers, fused_losses=fused)
        out, data = outs[0]
        ls = {k: float(v) for k, v in out["losses"].items()}
        pred = ts.last_preds[0]
        pose = pred["pose"] if layers == "all" else pred["pose"][-1:]
        ref = float(_ref_pose_loss(pose.detach(), pred["src_kp"][0], data["pose"][0].float()))
        assert abs(ls["pose"] - ref) <= 1e-5 * max(1.0, ref), (layers, ls["pose"], ref)
        rest = sum(ls[k] * LS.LOSS_WEIGHTS[k] for k in LS.LOSS_WEIGHTS)
        assert abs(ls["total"] - (rest + w * ls["pose"])) <= 1e-5 * max(1.0, abs(ls["total"])), (layers, ls)
        if fused:          # "last" keeps the executor's last-layer-only backward; "all" takes the full one
            assert calls == [layers == "last"], (layers, calls)
        assert all(torch.isfinite(p).all() for p in m.parameters())


def test_cli_flag_reaches_train_step(monkeypatch, tmp_path):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import train_nerf_regtr as T
    seen = {}

    class Stop(Exception):
        pass

    def fake(model, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(T, "TrainStep", fake)
    monkeypatch.setattr(sys, "argv", ["train_nerf_regtr.py", "--synthetic", "2", "--synthetic_res", "32", "--root_dir", str(tmp_path),
                                      "--pose_loss_weight", "0.5", "--pose_loss_layers", "all"])
    with pytest.raises(Stop):
        T.main()
    assert seen["pose_loss_weight"] == 0.5 and seen["pose_loss_layers"] == "all"
