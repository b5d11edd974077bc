"""The table of tests/losses_cases.py is sound and tests/losses_restatement.py is the project's loss formulation (no GPU): the restatement equals
losses.training_losses in torch fp64, values and gradients; the lattice cases are exact in fp32 and hold every edge they name; the generic cases'
decisions clear twice the fp32 error of their distances; every case reaches the kernel path it names; the GEMM descriptor tables stay inside
their buffers."""
import math
import struct

import numpy as np
import pytest
import torch

import losses_cases as C
import losses_restatement as LR
from dreg_nerf_amd import attn_ops as A, fused_losses as FL, lib as L, losses as LS

LIMIT = 2 ** 24


def _show(capsys, text):
    with capsys.disabled():
        print("\n    " + text, end="")


class _ForcedNeighbour(LS.InfoNCELoss):
    """InfoNCELoss with the neighbour index given: torch's topk leaves the choice among equal distances unspecified, the project's stated rule
    (csrc/losses.hip) is the lowest index, which is what the restatement hands in."""
    forced = None

    def forward(self, anchor_f, pos_f, anchor_xyz, pos_xyz):
        wt = torch.triu(self.W)
        logits = anchor_f @ (wt + wt.T) @ pos_f.T
        with torch.no_grad():
            dist = torch.cdist(anchor_xyz, pos_xyz, compute_mode="donot_use_mm_for_euclid_dist")
            i1 = self.forced[:, None]
            d1 = dist.gather(-1, i1)
            assert torch.equal(d1[:, 0], dist.min(-1).values)            # it IS a nearest one
            mask = d1[..., 0] < self.r_p
            ignore = dist < self.r_n
            ignore.scatter_(-1, i1, 0)
        logits = logits.masked_fill(ignore, -float("inf"))
        loss = -torch.gather(logits, -1, i1).squeeze(-1) + torch.logsumexp(logits, dim=-1)
        return torch.where(mask, loss, torch.zeros_like(loss)).sum() / mask.sum()


def _torch_fp64(c, robust, ref):
    """losses.training_losses per pair in fp64, mean over the pairs; gradients of the total with respect to cond, corr, ov."""
    t = lambda k: torch.from_numpy(np.array(c[k], dtype=np.float64))
    cond, corr, ov = (t(k).requires_grad_(True) for k in ("cond", "corr", "ov"))
    xyz, gt, tilde, poses = t("xyz"), t("gt"), t("tilde"), t("poses")
    forced = bool(c["tie_rows"])
    fl = (_ForcedNeighbour if forced else LS.InfoNCELoss)(256, float(np.float32(c["r_p"])), float(np.float32(c["r_n"]))).double()
    with torch.no_grad():
        fl.W.copy_(t("W"))
    P = len(c["segs"])
    tot, per = 0.0, np.zeros(5)
    for p, (s0, ns, t0, nt) in enumerate(c["segs"]):
        S, T = slice(s0, s0 + ns), slice(t0, t0 + nt)
        pred = {"src_feats": [cond[None, S]], "tgt_feats": [cond[None, T]], "src_kp": [xyz[S]], "tgt_kp": [xyz[T]],
                "src_kp_warped": [corr[None, S]], "tgt_kp_warped": [corr[None, T]], "src_overlap": [ov[None, S, None]], "tgt_overlap": [ov[None, T, None]]}
        if forced:
            fl.forced = torch.from_numpy(ref["dec"][p]["nn"])
        ls = LS.training_losses(pred, poses[p][None], fl, gt[:, S, None], gt[:, T, None], tilde[:, S, None], tilde[:, T, None], robust)
        per += np.array([float(ls[k].detach()) for k in FL.NAMES])
        # a pair without positives: its feature value is nan (kept in `per`), its gradient is 0 by the node's k = 0 rule where torch would spread nan
        keys = [k for k in LS.LOSS_WEIGHTS if not (k == "feature" and ref["dec"][p]["count"] == 0)]
        tot = tot + sum(ls[k] * LS.LOSS_WEIGHTS[k] for k in keys)
    (tot / P).backward()
    return per / P, cond.grad.numpy(), corr.grad.numpy(), ov.grad.numpy()


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    if m.any():
        assert float(np.abs(got[m] - want[m]).max()) <= rel * max(1.0, float(np.abs(want[m]).max()))


@pytest.mark.parametrize("robust", [False, True], ids=["l1", "robust"])
@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_equals_training_losses_in_fp64(name, robust):
    c, ref = C.build(name), C.reference(name, robust)
    per, g_cond, g_corr, g_ov = _torch_fp64(c, robust, ref)
    _close(ref["out"], per)
    _close(ref["d_cond"], g_cond)
    _close(ref["point"]["d_corr"], g_corr)
    _close(ref["point"]["d_ov"], g_ov)
    # a planted d = 0 is where the plain L1 takes the sub-gradient 0
    if not robust and c["kind"] == "lattice":
        z = ref["point"]["d"] == 0
        assert z.any() and not ref["point"]["d_corr"][z].any() and not g_corr[z].any()


def _edges(c, ref):
    r_p, r_n = float(np.float32(c["r_p"])), float(np.float32(c["r_n"]))
    e = dict(at_rp=0, at_rn=0, in_rp=0, out_rp=0, dist0=0, ties=0, zero_count=0, all_pos=0, one_pos=0)
    for d in ref["dec"]:
        e["at_rp"] += int((d["near"] == r_p).sum())
        e["in_rp"] += int((d["near"] == r_p - 1 / 64).sum())
        e["out_rp"] += int((d["near"] == r_p + 1 / 64).sum())
        e["at_rn"] += int((d["dist"] == r_n).sum())
        e["dist0"] += int((d["near"] == 0).sum())
        e["zero_count"] += int(d["count"] == 0)
        e["all_pos"] += int(d["count"] == len(d["nn"]))
        e["one_pos"] += int(d["count"] == 1)
    for (p, i, j, j2) in c["tie_rows"]:
        d, lg = ref["dec"][p], ref["fwd"][p]["logits"]
        if d["dist"][i, j] == d["dist"][i, j2] == d["near"][i] and d["nn"][i] == j and j < j2 and d["mask"][i] == 1 and abs(lg[i, j] - lg[i, j2]) > 0.05:       # four orders above the bound on loss_row
            e["ties"] += 1
    pt = ref["point"]
    e["d0"] = int((pt["d"] == 0).sum())
    e["d_max"] = float(np.abs(pt["d"]).max())
    e["zero_weight_sides"] = int((pt["partial"][:, 3] == 0).sum())
    return e


@pytest.mark.parametrize("name", list(C.LATTICE))
def test_lattice_cases_are_exact_and_hold_their_edges(name, capsys):
    c, ref = C.build(name), C.reference(name, False)
    f = {k: np.asarray(c[k], dtype=np.float64) for k in ("xyz", "poses", "cond", "W", "corr", "gt", "tilde")}
    ints = lambda a: np.array_equal(a, np.round(a))
    assert ints(f["xyz"] * 64) and float(np.abs(f["xyz"]).max()) <= 1.0
    assert ints(f["poses"][:, :3, :3]) and ints(f["poses"][:, :3, 3] * 64) and ints(f["corr"] * 64) and ints(f["cond"] * 16) and ints(f["W"])
    assert ints(f["tilde"] * 4) and set(np.unique(f["gt"])) <= {0.0, 1.0}
    worst = 0.0
    for p, (s0, ns, t0, nt) in enumerate(c["segs"]):
        Rm, t = f["poses"][p, :3, :3], f["poses"][p, :3, 3]
        if C.LATTICE[name].get("shear") != p:
            assert abs(np.linalg.det(Rm) - 1.0) < 1e-12 and np.array_equal(np.abs(Rm).sum(0), np.ones(3)) and np.array_equal(np.abs(Rm).sum(1), np.ones(3))
        # squared distances in units of 2^-12: the sum of the absolute values of every product that enters one
        a_abs = np.abs(f["xyz"][s0:s0 + ns]) @ np.abs(Rm).T + np.abs(t)
        q_abs = np.abs(f["xyz"][t0:t0 + nt])
        worst = max(worst, float((((a_abs[:, None] + q_abs[None]) * 64) ** 2).sum(-1).max()))
        assert ints(ref["dec"][p]["d2"] * 4096)
        # both maps of the point losses, in units of 1/64
        for M, rows in zip(LR.side_maps(f["poses"][p]), (slice(s0, s0 + ns), slice(t0, t0 + nt))):
            assert ints(M * 64)
            worst = max(worst, float(((np.abs(f["xyz"][rows]) @ np.abs(M[:, :3]).T + np.abs(M[:, 3]) + np.abs(f["corr"][rows])) * 64).max()))
        # dot products: q in units of 1/16, logits in units of 1/256
        ws = ref["wsym"]
        q_abs = (np.abs(f["cond"][s0:s0 + ns]) * 16) @ np.abs(ws)
        lg_abs = (np.abs(ref["fwd"][p]["q"]) * 16) @ (np.abs(f["cond"][t0:t0 + nt]) * 16).T
        assert ints(ref["fwd"][p]["q"] * 16) and ints(ref["fwd"][p]["logits"] * 256)
        worst = max(worst, float(q_abs.max()), float(lg_abs.max()))
        # and fp32 torch gives the fp64 logits bit for bit
        c32 = torch.from_numpy(np.array(c["cond"]))
        w32 = torch.from_numpy(ws.astype(np.float32))
        lg32 = (c32[s0:s0 + ns] @ w32) @ c32[t0:t0 + nt].T
        assert np.array_equal(lg32.numpy().astype(np.float64), ref["fwd"][p]["logits"])
    assert worst < LIMIT
    pt = ref["point"]
    assert ints(pt["d"] * 64) and ints(pt["partial"][:, 2] * 64) and ints(pt["partial"][:, 1] * 32) and float(pt["partial"][:, 1:3].max()) * 64 < LIMIT      # the sums are fp32 numbers
    e = _edges(c, ref)
    lgmax = max(float(np.abs(r["logits"]).max()) for r in ref["fwd"])
    _show(capsys, f"{name}: edges {e}; largest numerator / abs-sum {worst:.0f} of 2^24 = {LIMIT}; largest |logit| {lgmax:.2f}")
    for k, v in c["min_edges"].items():
        assert e[k] >= v, (k, e[k], v)
    if c["min_edges"].get("ties"):
        assert e["ties"] == len(c["tie_rows"])
    if name == "lat-shapes":
        assert e["dist0"] >= 1 and e["in_rp"] >= 1 and e["out_rp"] >= 1 and e["at_rn"] >= 1
    if name.startswith("lat-point") or name == "lat-131x70":
        assert e["d0"] >= 10 and 1.9 <= e["d_max"] <= 2.0
    if name == "lat-point-p3":
        # the source side of pair 0 is zero in every layer (factor 0); that of pair 2 only in the last (factor 1 / P, BCE from zeros)
        assert pt["partial"][0, 3] == 0 and pt["factor"][0] == 0 and pt["partial"][0, 2] > 0
        assert not np.asarray(c["gt"])[-1, c["segs"][2][0]:c["segs"][2][0] + 513].any() and pt["partial"][4, 3] > 0 and pt["factor"][4] == 1.0 / 3.0
        gt = np.asarray(c["gt"])
        assert all(not np.array_equal(gt[l], gt[l + 1]) for l in range(5))
        assert np.array_equal(f["poses"][1, :3, :3], C.SHEAR)


@pytest.mark.parametrize("name", list(C.GENERIC))
def test_generic_cases_decide_unambiguously(name, capsys):
    c, ref = C.build(name), C.reference(name, False)
    worst = []
    for d in ref["dec"]:
        m = LR.decision_margins(d, c["r_p"], c["r_n"])
        worst.append(min(m))
        assert min(m) > 1.0                      # every |dist - r| and every nearest / second gap clears 2 E: no row is left out of any comparison
        assert d["count"] > 0
    E = max(float(d["E"].max()) for d in ref["dec"])
    _show(capsys, f"{name}: smallest decision margin / 2E per pair {[f'{w:.1f}' for w in worst]} (largest E {E:.2e})")


def test_every_case_reaches_the_paths_it_names():
    nts = {seg[3] for n in C.INFONCE for seg in C.build(n)["segs"]}
    assert nts >= {1, 63, 64, 65, 257, 320, 2048, 2049} and any(nt % 4 for nt in nts)
    assert {math.ceil(nt / 64) for nt in nts} >= {1, 2, 5, 32, 33}                          # strided iterations of a lane: the unroll-by-4 loop's tails
    for n in C.INFONCE:
        for (s0, ns, t0, nt) in C.build(n)["segs"]:
            assert nt <= 2049 and (nt < 2048 or ns <= 8)
    shapes = C.build("lat-shapes")["segs"]
    wg = C.workgroups(shapes)
    assert wg[0] == (0, True, [0, 1, 1, 2]) and sum(s[1] for s in shapes) % 4 == 3
    wg = C.workgroups(C.build("lat-staging")["segs"])
    assert wg == [(0, True, [0, 0, 1, 1]),        # first pair staged, the later rows' own pair (2,049 targets) read from global memory
                  (1, False, [1, 2, 2, 3])]       # first pair not staged, the later rows' pairs (2,048 / 64 targets) read from global memory too
    wg = C.workgroups(C.build("gen-5x2049")["segs"])
    assert wg == [(0, False, [0, 0, 0, 0]), (0, False, [0, 1, 1, 1])]
    assert any(len(set(ps)) == 2 for _, _, ps in C.workgroups(C.build("lat-131x70")["segs"]))
    sides = {n for name in C.POINT for (_, ns, _, nt) in C.build(name)["segs"] for n in (ns, nt)}
    assert sides >= {1, 255, 256, 257, 513}
    assert {len(C.build(n)["segs"]) for n in C.POINT} >= {1, 3} and {C.build(n)["L"] for n in C.POINT} >= {1, 6}
    for name in C.NAMES:
        assert sum(ns + nt for _, ns, _, nt in C.build(name)["segs"]) <= 6300 and sum(s[1] for s in C.build(name)["segs"]) <= 1300


@pytest.mark.parametrize("name", C.NAMES)
def test_gemm_descriptor_tables_stay_inside_their_buffers(name):
    """fused_losses._gemm_tables over the case's segment list: pure host arithmetic over the packed records."""
    segs = C.build(name)["segs"]
    tab = A.ProblemTable([(ns, nt) for _, ns, _, nt in segs], torch.device("cpu"))
    assert tab.segs == segs
    R = tab.R
    size = {0: R * 256, 1: 256 * 256, 2: R * 256, 3: max(tab.total_logits, 1), 4: R * 256, 5: R * 256}
    nb = L.load().dreg_gemm_f32_desc_bytes()
    written = {}
    for level, (blob, n, tiles) in enumerate(FL._gemm_tables(tab, torch.device("cpu"))):
        raw = bytes(blob.tolist())
        assert len(raw) == n * nb and n == len(segs) * (2 if level == 2 else 1)
        run = 0
        for k in range(n):
            a, b, c_, tA, tB, M, N, K, lda, ldb, ldc, tile0, ao, bo, co = struct.unpack("<12i3q", raw[k * nb:(k + 1) * nb])
            assert tile0 == run and min(M, N, K) >= 1
            run += -(-M // 64) * -(-N // 64)
            for ident, off, rows, cols, ld in ((a, ao, K if tA else M, M if tA else K, lda), (b, bo, N if tB else K, K if tB else N, ldb), (c_, co, M, N, ldc)):
                assert ld >= cols and off >= 0 and off + (rows - 1) * ld + cols <= size[ident], (level, k, ident)
            span = (c_, co, co + (M - 1) * ldc + N)
            for other in written.get(level, []):                                       # outputs of one launch do not overlap
                assert other[0] != span[0] or other[2] <= span[1] or span[2] <= other[1]
            written.setdefault(level, []).append(span)
        assert run == tiles
    assert len(written[1]) == len(segs) and all(w[0] == 3 for w in written[1])
