"""GPU: the kernels of csrc/losses.hip, one C-ABI entry at a time and then through the autograd node, against the fp64 restatement of
tests/losses_restatement.py on the cases of tests/losses_cases.py (which tests/test_losses_host.py proves sound on the CPU).  Discrete results and
everything the lattice cases make exact are compared for equality; the rest against bounds the restatement derives from the kernels' operation counts.
Every bounded comparison prints its largest error / bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import losses_cases as C  # noqa: E402
import losses_restatement as LR  # noqa: E402
from dreg_nerf_amd import attn_ops as A, fused_losses as FL, lib as L, losses as LS, ops  # noqa: E402

DEV = "cuda:0"
U = LR.U
W = LS.LOSS_WEIGHTS
WO, WC, WF, WR = W["overlap"], W["nerf_cont"], W["feature"], W["corr"]
_DEVICE = {}


def _dev(name):
    """The case's arrays on the device (uploaded once, never written) and its row-space table."""
    if name not in _DEVICE:
        c = C.build(name)
        d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ("xyz", "poses", "cond", "W", "gt", "tilde", "ov", "corr")}
        d["tab"] = A.ProblemTable([(ns, nt) for _, ns, _, nt in c["segs"]], torch.device(DEV))
        assert d["tab"].segs == c["segs"]
        _DEVICE[name] = d
    return _DEVICE[name]


def _np(t):
    return t.detach().cpu().numpy()


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def _ratio(err, bound):
    """largest error / bound over the entries; entries with bound 0 must have error 0"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64) + np.zeros_like(err)
    assert not err[bound == 0].any()
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


def _report(what, name, value):
    print(f"[losses-fp64] {what} {name}: largest error / bound {value:.3f}")


# ------------------------------------------------------------------------------------------------------------------ neighbours, mask, count
def _run_nn(name):
    c, d = C.build(name), _dev(name)
    tab, P = d["tab"], len(c["segs"])
    nn = torch.full((tab.total_src,), -7, dtype=torch.int32, device=DEV)
    mask = torch.full((tab.total_src,), float("nan"), device=DEV)
    count = torch.full((P,), float("nan"), device=DEV)
    L.check(L.load().dreg_infonce_nn(L.ptr(d["xyz"]), L.ptr(d["poses"]), L.ptr(tab.pair_probs), L.ptr(tab.src_off), L.ptr(nn), L.ptr(mask), L.ptr(count),
                                     P, tab.total_src, float(c["r_p"]), L.stream()), "dreg_infonce_nn")
    return _np(nn), _np(mask), _np(count)


@pytest.mark.parametrize("name", C.INFONCE)
def test_neighbours_mask_and_count_equal_the_restatement(name):
    """dreg_infonce_nn: exact equality of nn (the lowest index among equal squared distances, in one lane's strided loop and at every stage of the
    shuffle reduction), mask (strict < r_p, with rows AT r_p) and count, staged and unstaged, in workgroups that mix pairs."""
    ref = C.reference(name)
    nn, mask, count = _run_nn(name)
    want_nn = np.concatenate([d["nn"] for d in ref["dec"]])
    want_mask = np.concatenate([d["mask"] for d in ref["dec"]])
    assert np.array_equal(nn, want_nn), np.nonzero(nn != want_nn)
    assert np.array_equal(mask, want_mask.astype(np.float32)), np.nonzero(mask != want_mask)
    assert np.array_equal(count, np.array([d["count"] for d in ref["dec"]], dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ rows
def _row_inputs(name):
    """Logits supplied by the test (the fp64 products rounded to fp32: exact on lattice cases) in the node's padded layout with NaN in the pad columns,
    the restatement's nn / mask / count as the kernel's inputs, and the restatement of the rows on exactly those fp32 logits."""
    c, ref, d = C.build(name), C.reference(name), _dev(name)
    tab = d["tab"]
    buf = np.full(max(tab.total_logits, 1), np.nan, dtype=np.float32)
    rows = []
    scale = WF / len(c["segs"])
    for (s0, ns, t0, nt), lo, f, dec in zip(c["segs"], tab.logit_off_host, ref["fwd"], ref["dec"]):
        ld = (nt + 3) // 4 * 4
        lg32 = _f32(f["logits"])
        if c["kind"] == "lattice":
            assert np.array_equal(lg32.astype(np.float64), f["logits"])
        buf[lo:lo + ns * ld].reshape(ns, ld)[:, :nt] = lg32
        rows.append(LR.infonce_rows(lg32.astype(np.float64), dec, scale))
    nn = torch.from_numpy(np.concatenate([x["nn"] for x in ref["dec"]]).astype(np.int32)).to(DEV)
    mask = torch.from_numpy(np.concatenate([x["mask"] for x in ref["dec"]]).astype(np.float32)).to(DEV)
    count = torch.tensor([x["count"] for x in ref["dec"]], dtype=torch.float32, device=DEV)
    return buf, rows, nn, mask, count, float(np.float32(scale))


def _run_rows(name, logits, nn, mask, count, scale, write_grad):
    c, d = C.build(name), _dev(name)
    tab = d["tab"]
    loss_row = torch.full((tab.total_src,), float("nan"), device=DEV)
    L.check(L.load().dreg_infonce_rows(L.ptr(logits), L.ptr(d["xyz"]), L.ptr(d["poses"]), L.ptr(tab.pair_probs), L.ptr(tab.src_off), L.ptr(tab.logit_off),
                                       L.ptr(nn), L.ptr(mask), L.ptr(count), L.ptr(loss_row), len(c["segs"]), tab.total_src, float(c["r_n"]), scale,
                                       int(write_grad), L.stream()), "dreg_infonce_rows")
    return _np(loss_row)


@pytest.mark.parametrize("name", C.INFONCE)
def test_rows_loss_and_logits_gradient(name):
    """dreg_infonce_rows.  loss_row within B = (4 (ceil(nt / 64) + 6) + 4) 2^-24 max(1, |lse|, |logit[nn]|); gradient entries within B times the entry's
    softmax term plus one ulp of scale / count; exactly 0 in excluded columns (strict < r_n, with entries AT r_n), in rows without a positive and in a
    pair without positives; write_grad = 0 leaves the buffer bit for bit; the pad columns are never written."""
    c, d = C.build(name), _dev(name)
    buf, rows, nn, mask, count, scale = _row_inputs(name)
    logits = torch.from_numpy(buf).to(DEV)
    lr0 = _run_rows(name, logits, nn, mask, count, scale, 0)
    assert np.array_equal(_np(logits).view(np.int32), buf.view(np.int32))                    # untouched, NaN pads included
    lr1 = _run_rows(name, logits, nn, mask, count, scale, 1)
    assert np.array_equal(lr0.view(np.int32), lr1.view(np.int32))
    got = _np(logits)
    worst_l = worst_g = 0.0
    off = 0
    for (s0, ns, t0, nt), lo, r, dec in zip(c["segs"], d["tab"].logit_off_host, rows, C.reference(name)["dec"]):
        ld = (nt + 3) // 4 * 4
        blk = got[lo:lo + ns * ld].reshape(ns, ld)
        assert np.isnan(blk[:, nt:]).all()                                                  # pad columns nt..ld
        g = blk[:, :nt].astype(np.float64)
        lr = lr1[off:off + ns].astype(np.float64)
        off += ns
        assert np.isfinite(g).all() and np.isfinite(lr).all()
        worst_l = max(worst_l, _ratio(np.abs(lr - r["loss_row"]), np.where(dec["mask"] > 0, r["B"], 0.0)))
        worst_g = max(worst_g, _ratio(np.abs(g - r["grad"]), r["grad_bound"]))
        zero = ~dec["included"] | (dec["mask"] == 0)[:, None] | (dec["count"] == 0)
        assert not g[zero].any()
        assert not lr[dec["mask"] == 0].any()
    _report("loss_row", name, worst_l)
    _report("logits gradient", name, worst_g)
    assert worst_l <= 1.0 and worst_g <= 1.0


# ------------------------------------------------------------------------------------------------------------------ point losses, deferred form, final
def _run_point(name, robust, with_tilde):
    c, d = C.build(name), _dev(name)
    tab, P, Ln, R = d["tab"], len(c["segs"]), c["L"], d["xyz"].shape[0]
    partial = torch.full((2 * P, 4), float("nan"), device=DEV)
    d_ov = torch.full((R,), float("nan"), device=DEV)
    d_corr = torch.full((R, 3), float("nan"), device=DEV)
    L.check(L.load().dreg_reg_point_losses(L.ptr(d["gt"]), L.ptr(d["tilde"]) if with_tilde else None, L.ptr(d["ov"]), L.ptr(d["corr"]), L.ptr(d["xyz"]),
                                           L.ptr(d["poses"]), L.ptr(tab.pair_probs), L.ptr(partial), L.ptr(d_ov), L.ptr(d_corr), Ln, R, P, int(robust),
                                           1e-6, WO, WR, L.stream()), "dreg_reg_point_losses")
    return partial, d_ov, d_corr


def _run_final(name, partial, loss_row, count):
    c, d = C.build(name), _dev(name)
    tab = d["tab"]
    out = torch.full((5,), float("nan"), device=DEV)
    L.check(L.load().dreg_reg_losses_final(L.ptr(partial), L.ptr(loss_row), L.ptr(count), L.ptr(tab.pair_probs), L.ptr(tab.src_off), L.ptr(out),
                                           len(c["segs"]), c["L"], 1e-6, WO, WC, WF, WR, L.stream()), "dreg_reg_losses_final")
    return out


def _check_point(name, robust, partial, d_ov, d_corr, tag):
    """partial [2P,4], d_ov, d_corr (numpy) of the kernel against the restatement; shared by the stage test and the end-to-end test."""
    c, pt = C.build(name), C.reference(name, robust)["point"]
    lattice = c["kind"] == "lattice"
    assert WR == 1.0 and WO == 1.0                                   # the factor then rounds once (the division by P)
    want = pt["partial"]
    assert np.array_equal(partial[:, 3], _f32(want[:, 3]))                                  # label sums: integers
    assert np.array_equal(partial[:, 1], _f32(want[:, 1]))                                  # smooth-L1: sums of 32nds (lattice) or of halves ({0,1} labels)
    _report(f"BCE partial ({tag})", name, _ratio(np.abs(partial[:, 0] - want[:, 0]), pt["bce_bound"]))
    assert _ratio(np.abs(partial[:, 0] - want[:, 0]), pt["bce_bound"]) <= 1.0
    if lattice and not robust:
        assert np.array_equal(partial[:, 2], _f32(want[:, 2]))                              # error sums: exact in the fp64 accumulators
    else:
        r = _ratio(np.abs(partial[:, 2] - want[:, 2]), pt["err_bound"])
        _report(f"error partial ({tag}, robust={int(robust)})", name, r)
        assert r <= 1.0
    _check_point_grads(name, robust, d_ov, d_corr, tag)


def _check_point_grads(name, robust, d_ov, d_corr, tag):
    c, pt = C.build(name), C.reference(name, robust)["point"]
    lattice = c["kind"] == "lattice"
    r = _ratio(np.abs(d_ov - pt["d_ov"]), 3 * 2 * U * np.abs(pt["d_ov"]))                   # 3 ulp
    _report(f"d_ov ({tag})", name, r)
    assert r <= 1.0
    fac32 = _f32(pt["factor"])
    for p, (s0, ns, t0, nt) in enumerate(c["segs"]):
        for side, rows in enumerate((slice(s0, s0 + ns), slice(t0, t0 + nt))):
            got, f = d_corr[rows], fac32[2 * p + side]
            if pt["factor"][2 * p + side] == 0:
                assert not got.any() and pt["partial"][2 * p + side, 3] == 0                # the zero-weight side: value and gradient 0
                continue
            if not robust:
                sure = np.ones_like(got, dtype=bool) if lattice else np.abs(pt["d"][rows]) > LR.map_error(LR.side_maps(c["poses"][p])[side], c["xyz"][rows]) + U * np.abs(pt["d"][rows])
                assert sure.mean() > 0.99
                assert np.array_equal(got[sure], (np.sign(pt["d"][rows]).astype(np.float32) * f)[sure])      # sign(d) * factor exactly, 0 at d = 0
    if robust:
        r = _ratio(np.abs(d_corr - pt["d_corr"]), pt["d_corr_bound"])
        _report(f"d_corr ({tag}, robust)", name, r)
        assert r <= 1.0


@pytest.mark.parametrize("robust", [False, True], ids=["l1", "robust"])
@pytest.mark.parametrize("name", C.POINT)
def test_point_losses_and_deferred_nerf_cont(name, robust):
    """dreg_reg_point_losses and dreg_nerf_cont_deferred.  Exact: label sums; on lattice cases the smooth-L1 and plain-L1 error partials (fp64 rounded
    to fp32), d_corr = sign(d) * factor with 0 at d = 0, value and gradient 0 on the zero-weight side; the deferred form's partial[.][1], out[1], out[4]
    against the one-call form.  Bounded: the BCE partial (its three roundings, expf, log1pf per row), d_ov (3 ulp), the robust values and derivatives."""
    c, ref = C.build(name), C.reference(name, robust)
    partial, d_ov, d_corr = _run_point(name, robust, True)
    _check_point(name, robust, _np(partial), _np(d_ov), _np(d_corr), "stage")
    # the final kernel on these partials, with loss rows and counts from the restatement
    loss_row = torch.from_numpy(_f32(np.concatenate([r["loss_row"] for r in ref["rows"]]))).to(DEV)
    count = torch.tensor([x["count"] for x in ref["dec"]], dtype=torch.float32, device=DEV)
    out = _run_final(name, partial, loss_row, count)
    # deferred: the first half leaves column 1 and nerf_cont at 0, the second half completes them bit for bit
    partial2, d_ov2, d_corr2 = _run_point(name, robust, False)
    p2 = _np(partial2)
    assert not p2[:, 1].any() and np.array_equal(p2[:, [0, 2, 3]].view(np.int32), _np(partial)[:, [0, 2, 3]].view(np.int32))
    assert torch.equal(d_ov2, d_ov) and torch.equal(d_corr2, d_corr)
    out2 = _run_final(name, partial2, loss_row, count)
    assert float(out2[1]) == 0.0 and np.array_equal(_np(out2)[[0, 2, 3]].view(np.int32), _np(out)[[0, 2, 3]].view(np.int32))
    d = _dev(name)
    L.check(L.load().dreg_nerf_cont_deferred(L.ptr(d["gt"]), L.ptr(d["tilde"]), L.ptr(d["tab"].pair_probs), L.ptr(partial2), L.ptr(out2), len(c["segs"]),
                                             c["L"], d["xyz"].shape[0], WO, WC, WF, WR, L.stream()), "dreg_nerf_cont_deferred")
    assert np.array_equal(_np(partial2).view(np.int32), _np(partial).view(np.int32))
    assert np.array_equal(_np(out2).view(np.int32), _np(out).view(np.int32))
    assert np.array_equal(_np(partial2)[:, 1], _f32(ref["point"]["partial"][:, 1]))
    want = LR.final(_np(partial), [_f32(r["loss_row"]) for r in ref["rows"]], [x["count"] for x in ref["dec"]], c["segs"], c["L"])
    assert abs(float(out[1]) - want[1]) <= U * abs(want[1])


@pytest.mark.parametrize("name", ["lat-shapes", "lat-131x70", "gen-131x300", "lat-point-p3"])
def test_final_means_on_the_kernels_own_partials(name):
    """dreg_reg_losses_final: the five outputs against the restatement evaluated on the kernel's own partials, within the fp32 output rounding; feature and
    total are NaN exactly when a pair has no positive, the other three stay finite."""
    c, ref = C.build(name), C.reference(name)
    partial, _, _ = _run_point(name, False, True)
    lrs = [_f32(r["loss_row"]) for r in ref["rows"]]
    counts = [x["count"] for x in ref["dec"]]
    out = _np(_run_final(name, partial, torch.from_numpy(np.concatenate(lrs)).to(DEV), torch.tensor(counts, dtype=torch.float32, device=DEV))).astype(np.float64)
    want = LR.final(_np(partial), lrs, counts, c["segs"], c["L"])
    nan = any(k == 0 for k in counts)
    assert nan == (name == "lat-shapes")
    assert np.isnan(out[2]) == nan and np.isnan(out[4]) == nan and np.isnan(want[2]) == nan
    assert np.isfinite(out[[0, 1, 3]]).all()
    for k in (0, 1, 3) if nan else (0, 1, 2, 3):
        assert abs(out[k] - want[k]) <= U * abs(want[k]), (k, out[k], want[k])
    if not nan:
        tot, b = LR.total_of(out[:4])
        assert abs(out[4] - tot) <= b


# ------------------------------------------------------------------------------------------------------------------ Wsym and its cache
@pytest.mark.parametrize("name", ["lat-131x70", "gen-131x300"])
def test_wsym_bit_for_bit(name):
    """dreg_infonce_wsym = triu(W) + triu(W)^T: one addition of x + 0 or of x + x per entry, exact; the diagonal doubled."""
    w = _dev(name)["W"]
    out = torch.full((256, 256), float("nan"), device=DEV)
    L.check(L.load().dreg_infonce_wsym(L.ptr(w), L.ptr(out), 256, L.stream()), "dreg_infonce_wsym")
    want = LR.wsym(C.build(name)["W"])
    got = _np(out)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(np.diag(got), 2 * np.diag(C.build(name)["W"])) and np.diag(got).any()


def test_wsym_cache_recomputes_when_w_changes_and_only_then():
    w = torch.nn.Parameter(_dev("lat-131x70")["W"].clone())
    a = FL._wsym(w)
    assert FL._wsym(w).data_ptr() == a.data_ptr() and FL._wsym(w) is a                      # no change: the cached tensor
    with torch.no_grad():
        w.copy_(_dev("gen-131x300")["W"])                                                   # bumps the version counter
    b = FL._wsym(w)
    assert b.data_ptr() != a.data_ptr()
    assert np.array_equal(_np(b).astype(np.float64), LR.wsym(C.build("gen-131x300")["W"]))
    assert FL._wsym(w) is b
    w.data[0, 0] = 5.0                                                                      # behind the version counter: the writer's duty
    assert FL._wsym(w) is b
    ops.bump_weight_generation()
    c = FL._wsym(w)
    assert c.data_ptr() != b.data_ptr() and float(c[0, 0]) == 10.0
    assert FL._wsym(w) is c


def test_wsym_cache_tells_a_new_parameter_from_a_freed_one():
    """A parameter allocated after another was freed usually gets its address, and after the same number of in-place writes its version counter: the
    cache must still see a different tensor (found by the end-to-end cases below, which build one InfoNCELoss each: the second one trained on the
    first one's Wsym)."""
    for name in ("lat-131x70", "gen-131x300", "lat-131x70"):
        w = torch.nn.Parameter(torch.empty(256, 256, device=DEV))
        with torch.no_grad():
            w.copy_(_dev(name)["W"])
        assert np.array_equal(_np(FL._wsym(w)).astype(np.float64), LR.wsym(C.build(name)["W"]))
        del w


# ------------------------------------------------------------------------------------------------------------------ the autograd node
def _node(name, robust, grads=True, factor=1.0):
    c, d = C.build(name), _dev(name)
    fl = LS.InfoNCELoss(256, c["r_p"], c["r_n"]).to(DEV)
    with torch.no_grad():
        fl.W.copy_(d["W"])
    cond, corr, ov = (d[k].clone().requires_grad_(grads) for k in ("cond", "corr", "ov"))
    bt = {"cond_last": cond, "corr_last": corr, "ov_last": ov[:, None], "xyz": d["xyz"], "tab": d["tab"]}
    out = FL.regtr_losses(bt, d["poses"], fl, d["gt"], d["tilde"], robust)
    if grads:
        (factor * out["total"]).backward()
    vals = np.array([float(out[k].detach()) for k in FL.NAMES], dtype=np.float32)
    return vals, (cond.grad, corr.grad, ov.grad) if grads else None, fl.W.grad, out["total"].requires_grad


@pytest.mark.parametrize("name,robust", [(n, False) for n in C.END_TO_END] + [("lat-point-p3", True)])
def test_autograd_node_end_to_end(name, robust):
    """FL.regtr_losses once, forward and backward.  Values: corr and nerf_cont exact on lattice cases (plain L1), overlap within the BCE bound, feature within
    the rows' bounds (plus twice the logits' GEMM bound on generic cases), NaN exactly for a pair without positives.  Gradients: d_corr and d_ov as in the
    stage test; d_cond within the restatement's running GEMM bound carried through levels 2 and 3; (3 * total).backward() gives exactly three times the
    gradients; the values without any requires_grad input equal those with, bit for bit; W.grad stays None (quirk Q5)."""
    c, ref = C.build(name), C.reference(name, robust)
    segs, P, Ln = c["segs"], len(c["segs"]), c["L"]
    vals, (g_cond, g_corr, g_ov), w_grad, rg = _node(name, robust)
    assert w_grad is None and rg
    pt, want = ref["point"], ref["out"]
    lattice = c["kind"] == "lattice"
    nan = any(x["count"] == 0 for x in ref["dec"])
    assert np.isnan(vals[2]) == nan and np.isnan(vals[4]) == nan and np.isfinite(vals[[0, 1, 3]]).all()
    n = np.array([ns + nt for _, ns, _, nt in segs], dtype=np.float64)
    b_ov = float(((pt["bce_bound"][0::2] + pt["bce_bound"][1::2]) / n).sum()) / P + U * abs(want[0])
    r = abs(vals[0] - want[0]) / b_ov
    _report("overlap (node)", name, r)
    assert r <= 1.0
    assert vals[1] == np.float32(want[1])                             # exact partials, the same fp64 expression, one output rounding
    if lattice and not robust:
        assert vals[3] == np.float32(want[3])
    if robust or not lattice:
        ratio = pt["partial"][:, 3] / np.maximum(pt["partial"][:, 3], LR.EPS)
        b = float((pt["err_bound"] * ratio).sum()) / P + 4 * U * abs(want[3])
        r = abs(vals[3] - want[3]) / b
        _report(f"corr (node, robust={int(robust)})", name, r)
        assert r <= 1.0
    if not nan:
        b = 0.0
        for f, rw, dec in zip(ref["fwd"], ref["rows"], ref["dec"]):
            delta = 0.0 if lattice else np.where(dec["included"], f["elogits"], 0.0).max(1)
            b += float((dec["mask"] * (rw["B"] + 2 * delta)).sum()) / dec["count"]
        b = b / P + 2 * U * abs(want[2])
        r = abs(vals[2] - want[2]) / b
        _report("feature (node)", name, r)
        assert r <= 1.0
        tot, tb = LR.total_of(vals[:4].astype(np.float64))
        assert abs(vals[4] - tot) <= tb
    # gradients
    _check_point_grads(name, robust, _np(g_ov), _np(g_corr), "node")
    g_cond_n = _np(g_cond).astype(np.float64)
    assert np.isfinite(g_cond_n).all()
    r = _ratio(np.abs(g_cond_n - ref["d_cond"]), ref["e_cond"])
    _report("d_cond (node)", name, r)
    assert r <= 1.0
    print(f"[losses-fp64] d_cond (node) {name}: largest bound {float(ref['e_cond'].max()):.2e} against largest |d_cond| {float(np.abs(ref['d_cond']).max()):.2e}")
    assert float(np.abs(g_cond_n).max()) > 0
    # an upstream factor other than 1
    vals3, (g3_cond, g3_corr, g3_ov), _, _ = _node(name, robust, factor=3.0)
    assert np.array_equal(vals3.view(np.int32), vals.view(np.int32))
    assert torch.equal(g3_cond, 3.0 * g_cond) and torch.equal(g3_corr, 3.0 * g_corr) and torch.equal(g3_ov, 3.0 * g_ov)
    # no input needs a gradient: write_grad = 0, levels 2 and 3 skipped, the same values
    vals0, _, _, rg0 = _node(name, robust, grads=False)
    assert np.array_equal(vals0.view(np.int32), vals.view(np.int32))
