"""GPU: the training backward of csrc/render_train.hip (ngp_render_bwd_kernel, fb_reduce_kernel) against the fp64 restatement of
tests/render_bwd_restatement.py, element by element, on the flat planted field of tests/render_bwd_cases.py.

On that field the encoding, both nets' activations and the colour are constants that fp32 and fp16 hold exactly, so the forward supplies
facts (the kept sets of tests/march_restatement.py, one alpha measured from a one-sample ray) and only the backward's own arithmetic is
under test: the compositing adjoint, the three ReLU masks, every MFMA tile of the five outer products, the 15 + k column mapping, and
scale, corner, hash index and trilinear weight of every level through the table gradient.  Every element of the five matrices and every
touched table entry must satisfy |gpu - fp64| <= (C + n) 2^-24 M: M the sum of the absolute values of the element's terms, n the number of
terms accumulated into it (each accumulation — MFMA, slab, chunk reduction, atomic — merges two partial sums: n - 1 roundings in all), C the
fp32 roundings on the longest path from a term to the element, counted below.  Rays whose kept set a rounding could change (Marched.decidable
false) carry g = 0 on both sides.  tests/test_render_bwd_host.py shows that fourteen deliberate errors each exceed 4 x this bound.

Not observable: the clamp of trunc_exp at h0 - 1 > 15 (a saturated sample has dL/dsigma = 0 and hides everything behind it)."""
import math

import numpy as np
import pytest
import torch

import march_cases as C
import ngp_grad_restatement as GR
import render_bwd_cases as B
import render_bwd_restatement as RB

gpu = pytest.mark.gpu
U = 2.0 ** -24

# fp32 roundings on the longest path from a term to an element, counted from ngp_render_bwd_kernel, march_composite (march.h) and the
# forward's rgb (render.hip); K = the largest number of in-model survivors of a ray of the launch.  Products of an fp32 and an fp16 value
# round once; 1 - c is exact (c is fp16 in [2^-3, 1)); h0 - 1 is exact (h0 is a dyadic fp16).
#   T_s *= (1 - alpha)                                     K      once per survivor before the sample
#   w = alpha T_s                                          1
#   forward rgb = sum w c + bkgd (1 - sum w)               3      beyond w and the K additions of a sum (counted with T: term j passes
#                                                                 j products of T and K - j additions).  The longest way is through the
#                                                                 opacity: 1 - opacity, * bkgd, the final +.  Through sum w c it is 2 (the
#                                                                 product w * c, rounded on its own: the build sets -ffp-contract=off, no
#                                                                 FMA is assumed anywhere in this table, and the final +); the backward's
#                                                                 own acc += w * c is 1 (the product) and lies on a path of its own
#   C - acc, T_s c - (..), gr *, dsig += (3 channels)      6
#   a.dt * dsig, * __expf(..)                              2
#   __expf(x) = v_exp_f32(x * log2(e))                     2 + 2 ceil|x|   v_exp_f32: 1 ulp = 2 units of 2^-24 ("AMD Instinct CDNA4 Instruction Set
#                                                                 Architecture Reference Guide", V_EXP_F32: "1 ULP accuracy"); the rounded
#                                                                 constant and the rounded product move its argument by 2 * 2^-24 relative,
#                                                                 the result by 2 |x| 2^-24 relative; x = h0 - 1
#   dO = w * gr * c * (1 - c)                              3      (v_rcp_f32 and the sigmoid's __expf sit before the fp16 rounding of c, which the
#                                                                 restated c is >= 8 * 2^-24 away from changing)
#   outer product term (MFMA)                              1      each of the five matrices
#   d2 = 3 products, 2 additions                           3
#   d1 = sum_j wc2[j][i] d2[j]                            65      a product and 64 additions
#   dout[k] = sum_i wc1[i][15 + k] d1[i]                  65
#   dh = sum_k wd2[k][i] dout[k]                          17
#   de = sum_i wd1[i][k] dh[i]                            65
#   wt = (1 - w) * . * .,  wt * de                         4      one subtraction on the path, two products, the product with de
def counts(K, h0):
    w = K + 1
    dsig = w + 3 + 6
    dh0 = dsig + 2 + 2 + 2 * math.ceil(abs(h0 - 1.0))
    dO = w + 3
    d2 = dO + 3
    d1 = d2 + 65
    dout = d1 + 65
    dh = max(dh0, dout) + 17
    de = dh + 65
    return {"c3": dO + 1, "c2": d2 + 1, "c1": d1 + 1, "d2_row0": dh0 + 1, "d2": dout + 1, "d1": dh + 1, "table": de + 4}


def bounds(res, K, h0):
    """The bound per element: dict over the five matrices and "table" (aligned with res.t_idx)."""
    c = counts(K, h0)
    b = {k: (c[k] + res.n[k]) * U * res.M[k] for k in ("c3", "c2", "c1", "d1")}
    cd2 = np.full((16, 1), float(c["d2"]))
    cd2[0] = c["d2_row0"]
    b["d2"] = (cd2 + res.n["d2"]) * U * res.M["d2"]
    b["c1"][:, :16] += 2.0 ** -11 * res.M["c1"][:, :16]               # the kernel's fp16 SH value may differ from the oracle's by an ulp
    b["table"] = (c["table"] + res.t_n) * U * res.t_M
    return b


# ------------------------------------------------------------------------------------------------------------------------------ the GPU side
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


_FIELDS = {}


def _field(dev, dens, model):
    from dreg_nerf_amd import ngp
    if dens not in _FIELDS:
        p = B.planted(dens)
        f = ngp.NGPradianceField(C.EXACT_MODEL)
        with torch.no_grad():
            f.mlp_base.params.copy_(torch.from_numpy(p["base"]))
            f.color_mlp.params.copy_(torch.from_numpy(p["color"]))
        _FIELDS.clear()                                               # one 12.6 M-parameter field on the device at a time
        _FIELDS[dens] = f.to(dev)
    f = _FIELDS[dens]
    with torch.no_grad():
        f.aabb.copy_(torch.tensor(model, dtype=torch.float32))
    return f


def _grid(case, dev):
    from dreg_nerf_amd import render as R, visibility
    b8 = torch.from_numpy(case.binary).to(dev).to(torch.uint8).contiguous()
    return R.BlockGrid(case.roi, b8, visibility.coarse_occupancy_bits(b8))


_ALPHA = {}


def _alpha(dev, dens):
    """The kernel's alpha: the opacity of a ray that keeps exactly one sample (the forward is not under test; it supplies this fact)."""
    if dens not in _ALPHA:
        from dreg_nerf_amd import render as R
        c = C.calibration_case(B.DT)
        assert c.ref.n_kept.tolist() == [1]
        f = _field(dev, dens, c.model).eval()
        with torch.no_grad():
            out = R.render_image(f, _grid(c, dev), R.Rays(torch.from_numpy(c.o).to(dev), torch.from_numpy(c.d).to(dev)), c.scene, near_plane=c.near,
                                 far_plane=c.far, render_step_size=c.dt, render_bkgd=torch.tensor(B.BKGD))
        a = float(out[1].reshape(-1)[0])
        a64 = B.alpha64(B.H0[dens])
        print(f"{dens}: a_gpu {a!r}, a_fp64 {a64!r}, difference {a - a64:.3e}")
        assert abs(a - a64) <= 4 * U
        col = out[0].reshape(-1).cpu().double().numpy()
        want = B.planted(dens)["c"] * a + np.array(B.BKGD) * (1.0 - a)
        assert np.abs(col - want).max() <= 8 * U, (col, want)          # the planted colour is what the forward renders
        _ALPHA[dens] = a
    return _ALPHA[dens]


def _backward(dev, dens, case, g):
    """(grad of mlp_base.params, grad of color_mlp.params) as fp64 numpy, through render_image_train(...).backward."""
    from dreg_nerf_amd import ngp_train, render as R
    f = _field(dev, dens, case.model).train()
    f.mlp_base.params.grad = None
    f.color_mlp.params.grad = None
    rays = R.Rays(torch.from_numpy(case.o).to(dev), torch.from_numpy(case.d).to(dev))
    rgb, _, _, ns = ngp_train.render_image_train(f, _grid(case, dev), rays, case.scene, case.dt, torch.tensor(B.BKGD), jitter=torch.from_numpy(case.jitter).to(dev))
    (rgb * torch.from_numpy(g).to(dev)).sum().backward()
    return f.mlp_base.params.grad.cpu().numpy(), f.color_mlp.params.grad.cpu().numpy(), ns


def _compare(dev, dens, case, label):
    a = _alpha(dev, dens)
    q = float(np.float32(1) - np.float32(a))
    r = case.ref
    g = B.g_rgb_of(case) * r.decidable[:, None]
    p = B.planted(dens)
    levels = GR.levels_from_ctypes(_field(dev, dens, case.model)._levels)       # the kernel's own level table (dreg_ngp_level_table)
    res = RB.backward64(B.record_of(p, case, r), p["weights"], r, a, q, g, B.BKGD, case.dt, levels, case.model)
    assert res.firm[r.n_kept > 0].all()                                 # (tests/test_render_bwd_host.py: no accepted alpha has an undecidable stop)
    gb, gc, ns = _backward(dev, dens, case, g)
    if r.decidable.all():
        assert ns == int(res.surv.sum())
    K = int(r.n_model.max())
    bnd = bounds(res, K, B.H0[dens])
    got = {"d1": gb[:2048].reshape(64, 32), "d2": gb[2048:3072].reshape(16, 64), "c1": gc[:2048].reshape(64, 32),
           "c2": gc[2048:6144].reshape(64, 64), "c3": gc[6144:6144 + 192].reshape(3, 64)}
    assert not gc[6144 + 192:].any()                                    # padding rows 3..15 of colour W3
    tab = gb[3072:].copy()
    got_t = tab[res.t_idx].astype(np.float64)
    tab[res.t_idx] = 0.0
    stray = np.nonzero(tab)[0]
    assert len(stray) == 0, (len(stray), stray[:16].tolist(), tab[stray[:16]].tolist())      # untouched entries are exactly 0
    ratios = {}
    blocks = [(k, got[k].astype(np.float64), res.val[k], bnd[k]) for k in RB.MATRICES]
    blocks.insert(3, ("c1 sh", blocks[2][1][:, :16], blocks[2][2][:, :16], blocks[2][3][:, :16]))
    blocks[2] = ("c1 feat+1", blocks[2][1][:, 16:], blocks[2][2][:, 16:], blocks[2][3][:, 16:])
    for l in range(16):
        s = res.t_level == l
        blocks.append((f"table {l}", got_t[s], res.t_val[s], bnd["table"][s]))
    for name, x, want, b in blocks:
        err = np.abs(x - want)
        assert np.all(x[b == 0] == 0), name                             # no term: exactly 0
        ratios[name] = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    line = ", ".join(f"{k} {v:.2e}" for k, v in ratios.items())
    print(f"RATIO {label} {dens} (K {K}, {int(res.surv.sum())} survivors, {len(res.t_idx)} table elements): {line}")
    bad = {k: v for k, v in ratios.items() if v > 1.0}
    assert not bad, bad
    assert len(res.t_idx) > 0 and all(np.abs(got[k]).sum() > 0 for k in RB.MATRICES)


@gpu
@pytest.mark.parametrize("dens", ("thin", "dense"))
@pytest.mark.parametrize("j", range(len(C.JITTERS)), ids=[str(j) for j in C.JITTERS])
def test_flat_field_within_the_counted_roundings(dev, j, dens):
    _compare(dev, dens, B.planted_set(C.JITTERS[j]), f"ragged jitter {C.JITTERS[j]}")


@gpu
@pytest.mark.parametrize("dens", ("thin", "dense"))
@pytest.mark.parametrize("n", B.EDGE_COUNTS)
def test_lane_and_chunk_edges(dev, n, dens):
    _compare(dev, dens, B.edge_set(n), f"{n} rays")


@gpu
@pytest.mark.parametrize("dens", ("thin", "dense"))
def test_wide_launch_of_128_ray_chunks(dev, dens):
    """131,073 rays: the first launch whose chunks hold 128 rays; the rays that hit sit at 63, 64, 127, 128, the last index and between."""
    _compare(dev, dens, B.wide_set(), "131073 rays")


@gpu
def test_all_miss_launch_is_exactly_zero(dev):
    case = B.miss_set()
    gb, gc, ns = _backward(dev, "thin", case, B.g_rgb_of(case))
    assert ns == 0 and not gb.any() and not gc.any()


@gpu
def test_entry_point_accumulates_into_the_callers_buffers(dev):
    """dreg_ngp_render_bwd adds into grad_base / grad_color: two calls without zeroing give exactly twice the first call's MLP part (x + x is
    exact) and, within the reassociation of the fp32 atomics (the bound of test_backward_mlp_gradients_deterministic_across_runs_and_widths),
    twice its table part."""
    from dreg_nerf_amd import lib as L, ngp_train, render as R
    case = B.edge_set(129)
    f = _field(dev, "thin", case.model).train()
    lib = L.load()
    o, d, jit = (torch.from_numpy(v).to(dev) for v in (case.o, case.d, case.jitter))
    grid = _grid(case, dev)
    with torch.no_grad():
        rgb = ngp_train.render_image_train(f, grid, R.Rays(o, d), case.scene, case.dt, torch.tensor(B.BKGD), jitter=jit)[0].contiguous()
    g = torch.from_numpy(B.g_rgb_of(case)).to(dev)
    base16, col16 = f._prepared()
    roi, b8, bits = R._grid_parts(grid, dev)
    gb = torch.zeros(base16.numel(), dtype=torch.float32, device=dev)
    gc = torch.zeros(col16.numel(), dtype=torch.float32, device=dev)
    nws = int(lib.dreg_ngp_render_bwd_workspace_bytes(len(o)))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)

    def call():
        L.check(lib.dreg_ngp_render_bwd(L.ptr(o), L.ptr(d), L.ptr(jit), len(o), L.ptr(b8), b8.shape[0], b8.shape[1], b8.shape[2], L.ptr(bits),
                                        base16.data_ptr(), col16.data_ptr(), *f._levels, L.f6(roi), L.f6(case.scene), L.f6(f._aabb_host()),
                                        -math.inf, math.inf, case.dt, 0.0, 1e-4, L.ptr(rgb), L.ptr(g), L.ptr(gb), L.ptr(gc), L.ptr(ws), nws, L.stream()),
                "dreg_ngp_render_bwd")
        return gb.clone(), gc.clone()

    b1, c1 = call()
    b2, c2 = call()
    assert c1.abs().sum() > 0 and b1[:3072].abs().sum() > 0 and b1[3072:].abs().sum() > 0
    assert torch.equal(b2[:3072], 2 * b1[:3072]) and torch.equal(c2, 2 * c1)
    torch.testing.assert_close(b2[3072:], 2 * b1[3072:], rtol=1e-4, atol=1e-5 * float(b1[3072:].abs().max()))
