"""GPU: the row-panel kernels of the point-set half (csrc/pointset_panel.hip: GEMM -> LayerNorm forward or backward row pass -> GEMM in
one launch, a workgroup per 64 rows) against the three launches they replace, and the executor with and without panel launches.

Every check is an equality: the panel kernel forms each output element by the same in-order chain of MFMAs over K, rounds at the same
points and shares the LayerNorm row arithmetic with the stand-alone LayerNorm kernels, so no tolerance applies."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dreg_nerf_amd import attn_ops as A, lib as L, params, pointset_exec as PX  # noqa: E402
from dreg_nerf_amd.optim import FlatAdamW  # noqa: E402
from dreg_nerf_amd.regtr import NeRFRegTr  # noqa: E402

SPARE = 64          # rows behind every output, pre-filled: a panel's tail must not touch them
EPS = 1e-5


def _pack(lib, w):
    cout, cin = w.shape
    out = torch.empty(cout, lib.dreg_conv3d_kpad(1, cin, L.DT_BF16), dtype=torch.bfloat16, device=w.device)
    L.check(lib.dreg_pack_conv_weight(L.ptr(w), L.ptr(out), cout, cin, cin, 1, 0, L.DT_BF16, L.stream()), "dreg_pack_conv_weight")
    return out


def _linear(lib, x, wpk, bias, residual, out, rows, cin, cout, relu, out_f32):
    """The executor's linear_fwd: the 1x1x1 path of the implicit-GEMM kernels, split-K workspace offered."""
    nws = lib.dreg_conv3d_igemm_workspace_bytes(rows, 1, 1, 1, cin, 1, 1, 1, cout, 1, 1, 0, 0, 0, 0)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
    a = 1 if residual is not None else 0
    L.check(lib.dreg_conv3d_igemm_ws(L.ptr(x), L.ptr(wpk), L.ptr(out), L.ptr(bias), L.ptr(residual), rows, 1, 1, 1, cin, 1, 1, 1, cout, 1, 1, 0, 0,
                                     int(relu), a, a, a, a, 0, int(out_f32), L.ptr(ws) if nws else None, nws, L.stream()), "dreg_conv3d_igemm_ws")


def _outputs(R, N2, dev):
    """x, h, stats, out2 with SPARE sentinel rows behind the R real ones (and sentinels in the real rows: every one must be written)."""
    x = torch.full((R + SPARE, 256), -7.25, dtype=torch.float32, device=dev)
    h = torch.full((R + SPARE, 256), -3.5, dtype=torch.bfloat16, device=dev)
    st = torch.full((R + SPARE, 2), -9.0, dtype=torch.float32, device=dev)
    o = torch.full((R + SPARE, N2), -5.5, dtype=torch.bfloat16, device=dev)
    return x, h, st, o


@pytest.mark.parametrize("with_pe", [False, True])
@pytest.mark.parametrize("K1,N2,relu", [(256, 768, 0), (256, 1024, 1), (1024, 768, 0)])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 255])
def test_forward_panel_equals_its_three_launches(R, K1, N2, relu, with_pe):
    lib = L.load()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1000 * R + K1 + N2 + int(with_pe))
    rn = lambda *s: torch.randn(*s, generator=g)
    a1 = rn(R, K1).to(torch.bfloat16).to(dev)
    w1 = (rn(256, K1) * K1 ** -0.5).to(dev)
    w2 = (rn(N2, 256) / 16).to(dev)
    b1, b2 = (0.1 * rn(256)).to(dev), (0.5 * rn(N2)).to(dev)
    res = rn(R, 256).to(dev)
    gamma, beta = (1 + 0.1 * rn(256)).to(dev), (0.1 * rn(256)).to(dev)
    pe = rn(R, 256).to(dev) if with_pe else None
    p1, p2 = _pack(lib, w1), _pack(lib, w2)

    rx, rh, rst, ro = _outputs(R, N2, dev)
    _linear(lib, a1, p1, b1, res, rx, R, K1, 256, 0, 1)
    L.check(lib.dreg_layernorm_fwd(L.ptr(rx), L.ptr(gamma), L.ptr(beta), L.ptr(pe), L.ptr(rh), L.ptr(rst), R, 256, EPS, 0, L.stream()), "dreg_layernorm_fwd")
    _linear(lib, rh, p2, b2, None, ro, R, 256, N2, relu, 0)

    x, h, st, o = _outputs(R, N2, dev)
    L.check(lib.dreg_ps_panel_fwd(L.ptr(a1), L.ptr(p1), L.ptr(b1), L.ptr(res), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(pe), L.ptr(h), L.ptr(st),
                                  L.ptr(p2), L.ptr(b2), L.ptr(o), R, K1, N2, relu, EPS, L.stream()), "dreg_ps_panel_fwd")
    torch.cuda.synchronize()
    for name, got, ref in (("x", x, rx), ("h", h, rh), ("stats", st, rst), ("out2", o, ro)):
        assert torch.equal(got[:R], ref[:R]), f"{name} differs from the three-launch chain"
        assert torch.equal(got[R:], ref[R:]), f"{name}: rows behind the last one were written"
    assert float(ro[:R].float().abs().max()) > 0 and not bool((rx[:R] == -7.25).all())


def _pack_t(lib, w):
    """Data-gradient pack [cin][kpad(cout)] of a linear layer's weight [cout, cin]."""
    cout, cin = w.shape
    out = torch.empty(cin, lib.dreg_conv3d_kpad(1, cout, L.DT_BF16), dtype=torch.bfloat16, device=w.device)
    L.check(lib.dreg_pack_conv_weight(L.ptr(w), L.ptr(out), cout, cin, cin, 1, 1, L.DT_BF16, L.stream()), "dreg_pack_conv_weight")
    return out


def _dgrad(lib, g, wpk_t, gx, rows, cin, cout):
    """The executor's linear_dgrad: gx [rows, cin] = g [rows, cout] W."""
    nws = lib.dreg_conv3d_igemm_workspace_bytes(rows, 1, 1, 1, cout, 1, 1, 1, cin, 1, 1, 0, 1, 0, 0)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=g.device)
    L.check(lib.dreg_conv3d_igemm_ws(L.ptr(g), L.ptr(wpk_t), L.ptr(gx), None, None, rows, 1, 1, 1, cout, 1, 1, 1, cin, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0,
                                     L.ptr(ws) if nws else None, nws, L.stream()), "dreg_conv3d_igemm_ws")


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("K1,N2", [(768, 256), (1024, 256), (768, 0)])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 255])
def test_backward_panel_equals_its_three_launches(R, K1, N2, in_place):
    """in_place: a second by-passing gradient that IS the output (the previous layer's output gradient, accumulated in place)."""
    lib = L.load()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(2000 * R + K1 + N2 + int(in_place))
    rn = lambda *s: torch.randn(*s, generator=g)
    g1 = rn(R, K1).to(torch.bfloat16).to(dev)
    p1 = _pack_t(lib, (rn(K1, 256) * K1 ** -0.5).to(dev))
    p2 = _pack_t(lib, (rn(256, 256) / 16).to(dev)) if N2 else None
    x = (2 * rn(R, 256) + 0.5).to(dev)
    mean = x.mean(1, keepdim=True)
    stats = torch.cat([mean, 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS)], 1).contiguous()
    gamma = (1 + 0.1 * rn(256)).to(dev)
    dx_add = rn(R, 256).to(dev)
    prev = rn(R, 256)
    nblk = lib.dreg_layernorm_bwd_blocks(R)
    assert lib.dreg_layernorm_bwd_workspace_bytes(R) == nblk * 512 * 4

    def outputs():
        dx = torch.full((R + SPARE, 256), -7.25, dtype=torch.float32, device=dev)
        if in_place:
            dx[:R] = prev.to(dev)
        return (dx, torch.full((R + SPARE, 256), -3.5, dtype=torch.bfloat16, device=dev), torch.full(((nblk + 2) * 512,), -9.0, dtype=torch.float32, device=dev),
                torch.full((R + SPARE, 256), -5.5, dtype=torch.bfloat16, device=dev))

    rdx, rbf, rpart, ro = outputs()
    dH = torch.empty(R, 256, dtype=torch.bfloat16, device=dev)
    _dgrad(lib, g1, p1, dH, R, 256, K1)
    L.check(lib.dreg_layernorm_bwd_parts(L.ptr(x), L.ptr(dH), None, L.ptr(gamma), L.ptr(stats), L.ptr(rdx), L.ptr(dx_add), L.ptr(rdx) if in_place else None,
                                         L.ptr(rbf), L.ptr(rpart), R, 256, 0, L.stream()), "dreg_layernorm_bwd_parts")
    if N2:
        _dgrad(lib, rbf, p2, ro, R, 256, 256)

    dx, bf, part, o = outputs()
    L.check(lib.dreg_ps_panel_bwd(L.ptr(g1), L.ptr(p1), L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(dx_add), L.ptr(dx) if in_place else None, L.ptr(dx), L.ptr(bf),
                                  L.ptr(part), L.ptr(p2), L.ptr(o) if N2 else None, R, K1, N2, L.stream()), "dreg_ps_panel_bwd")
    torch.cuda.synchronize()
    for name, got, ref in (("dx", dx, rdx), ("dx_bf16", bf, rbf), ("out2", o, ro)):
        assert torch.equal(got[:R], ref[:R]), f"{name} differs from the three-launch chain"
        assert torch.equal(got[R:], ref[R:]), f"{name}: rows behind the last one were written"
    assert torch.equal(part, rpart), "dgamma / dbeta partials differ (or were written behind the last block)"
    assert float(rpart[:nblk * 512].abs().max()) > 0 and bool((rpart[nblk * 512:] == -9.0).all())


def test_panel_entry_point_rejects_shapes_it_does_not_cover():
    lib = L.load()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = L.ptr(t)
    call = lambda R, K1, N2: lib.dreg_ps_panel_fwd(p, p, p, p, p, p, p, None, p, p, p, p, p, R, K1, N2, 0, EPS, L.stream())
    assert call(0, 256, 768) != 0 and call(8, 96, 768) != 0 and call(8, 256, 128) != 0
    bwd = lambda R, K1, N2: lib.dreg_ps_panel_bwd(p, p, p, p, p, None, None, p, None, p, p, p, R, K1, N2, L.stream())
    assert bwd(0, 768, 256) != 0 and bwd(8, 100, 256) != 0 and bwd(8, 768, 512) != 0


# ---------------------------------------------------------------------------------------------- executor level
def _model():
    m = NeRFRegTr(precision="bf16")
    m.load_state_dict(params.synth_state_dict(0), strict=True)
    m = m.cuda().train()
    opt = FlatAdamW([p for p in m.parameters()])
    opt.zero_grad()
    return m, opt


@pytest.fixture(scope="module")
def model():
    return _model()


def _run(m, opt, segs, level, use=(True, True, True), last=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    R = sum(a + b for a, b in segs)
    feats = (0.5 * torch.randn(R, 256, generator=g)).cuda().requires_grad_(True)
    xyz = (torch.rand(R, 3, generator=g) * 2 - 1).cuda()
    w = [torch.randn(6, R, c, generator=g).cuda() for c in (256, 3, 1)]
    tab = A.ProblemTable(segs, torch.device("cuda"))
    A.set_precision("bf16")
    opt.zero_grad()
    P = m._P()
    keep = PX.PANEL
    PX.PANEL = level
    try:
        ex = PX.executor_for(m, P)
        assert ex is not None
        out = PX.encode_decode(ex, feats, xyz, m.position_embedding(xyz), tab, P["transformer_encoder.norm.weight"], with_last=True)
        src = out[3:] if last else tuple(t[-1] for t in out[:3])      # last: the *_last outputs (last_only backward)
        loss = 0.0
        for u, t, wt, s in zip(use, src, w, (1e-2, 1.0, 1.0)):
            if u:
                loss = loss + (t * wt[-1]).sum() * s
        if not last:
            for u, t, wt, s in zip(use, out[:3], w, (1e-2, 1.0, 1.0)):
                if u:
                    loss = loss + (t[:-1] * wt[:-1]).sum() * s
        loss.backward()
        torch.cuda.synchronize()
    finally:
        PX.PANEL = keep
    grads = {n: P[n].grad.detach().clone() for n in PX.param_names()}
    return [t.detach().clone() for t in out[:3]], feats.grad.detach().clone(), grads


def _same(a, b, what):
    for x, y, name in zip(a[0], b[0], ("cond", "corr", "ov")):
        assert torch.equal(x, y), f"{what}: {name} differs"
    assert torch.equal(a[1], b[1]), f"{what}: d_feats differs"
    bad = [n for n in b[2] if not torch.equal(a[2][n], b[2][n])]
    assert not bad, f"{what}: parameter gradients differ: {bad[:6]} ({len(bad)})"


@pytest.mark.parametrize("segs", [[(1, 2)], [(64, 64)], [(70, 55), (40, 90)]])
def test_executor_is_bit_identical_with_and_without_panels(model, segs):
    m, opt = model
    runs = [_run(m, opt, segs, level) for level in (3, 2, 1)]
    _same(runs[0], runs[2], "level 3 against level 1")
    _same(runs[1], runs[2], "level 2 against level 1")
    assert all(float(v.abs().max()) > 0 for v in runs[2][2].values())


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_single_head_gradients_with_panels(model, which, last):
    m, opt = model
    use = tuple(i == which for i in range(3))
    segs = [(70, 55), (40, 90)]
    runs = [_run(m, opt, segs, level, use=use, last=last, seed=5) for level in (3, 2, 1)]
    _same(runs[0], runs[2], "level 3 against level 1")
    _same(runs[1], runs[2], "level 2 against level 1")
