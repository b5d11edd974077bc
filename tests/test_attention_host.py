"""CPU: the restatement of the attention kernels' arithmetic (tests/attention_restatement.py) against a direct fp64 softmax(Q K^T s) V and its
autograd gradients on the case list of tests/test_hip_attention.py; every seeded defect of the restatement breaks the tolerance of that list on at
least one case (so the list and the tolerances can tell a subtly wrong kernel from a right one without a GPU); the closed forms of the q = 0 and
peaked regimes; ProblemTable's rejection of empty segments."""
import math

import pytest
import torch

import attention_restatement as AR

H = 2          # heads (32-channel form) / layers (xyz form): each is independent of the others
CASES = AR.case_list()
_CACHE = {}


def _case(idx, xyz, mode):
    """(inputs, fp64 reference, restatement result, restatement errors) of one case, computed once."""
    key = (idx, xyz, mode)
    if key not in _CACHE:
        name, kind, table, R, regime = CASES[idx]
        inp = AR.make_inputs(table, R, regime, xyz, mode, H, seed=1000 + idx)
        ref = AR.reference(*inp[:4], table, inp[4], xyz)
        got = AR.run(*inp[:4], table, inp[4], mode, xyz)
        _CACHE[key] = (inp, ref, got, AR.errors(got, ref, table, AR.compared_outputs(regime, xyz), AR.zero_scales(*inp)))
    return _CACHE[key]


def test_case_list_covers_every_length_and_tile_count():
    singles = [(t[0][1], t[0][3]) for _, kind, t, _, regime in CASES if kind == "single" and regime == "unit"]
    assert {a for a, _ in singles} >= set(AR.LENGTHS) and {b for _, b in singles} >= set(AR.LENGTHS)
    for side in (0, 1):
        tiles = {min(3, (s[side] + 63) // 64) for s in singles}
        assert tiles == {1, 2, 3}
    for must in ((1, 1), (1, 193), (193, 1), (1184, 1170)):
        assert must in singles
    for segs in AR.TABLES.values():
        sp, cp, R = AR.segs_tables(segs)
        lens = [p[1] for p in sp]
        assert lens.index(max(lens)) != 0                      # the max_len problem is not the first
    assert any(1 in pair and max(pair) >= 1184 for pair in AR.TABLES["one_next_to_long"])
    assert {r for *_, r in CASES} == set(AR.REGIMES)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("xyz", [False, True], ids=["mha", "xyz"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_restatement_matches_fp64(idx, xyz, mode):
    """Switches off: fp32 mode agrees with fp64 to fp32 rounding, bf16 mode stays inside the tolerance rule (so 4 x its error is a usable bound)."""
    name, kind, table, R, regime = CASES[idx]
    inp, ref, got, err = _case(idx, xyz, mode)
    if regime == "shift_neg":
        assert float(ref["lse"][torch.isfinite(ref["lse"])].max()) < -90.0
    if regime == "shift_pos":
        assert float(ref["lse"][torch.isfinite(ref["lse"])].min()) > 90.0
    for out, es in err.items():
        print(f"{name} {'xyz' if xyz else 'mha'} {mode} {out}: restatement error {max(es):.3e}")
        assert max(es) <= AR.CAP[mode], (name, out, max(es))


DEFECT_CASES = [i for i, c in enumerate(CASES) if c[3] <= 700]      # the small cases are enough (and quick): a subset of the same list


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("xyz", [False, True], ids=["mha", "xyz"])
@pytest.mark.parametrize("defect", AR.DEFECTS)
def test_every_seeded_defect_is_caught(defect, xyz, mode):
    """A kernel with this one defect would fail tests/test_hip_attention.py: on at least one case its error exceeds the case's bound."""
    caught = []
    for idx in DEFECT_CASES:
        name, kind, table, R, regime = CASES[idx]
        inp, ref, got, err = _case(idx, xyz, mode)
        bad = AR.run(*inp[:4], table, inp[4], mode, xyz, **{defect: True})
        berr = AR.errors(bad, ref, table, AR.compared_outputs(regime, xyz), AR.zero_scales(*inp))
        for out in berr:
            if max(berr[out]) > AR.bound(out, mode, xyz, err, ref, table):
                caught.append((name, out, max(berr[out])))
        if caught:
            break
    assert caught, f"no case of the list notices {defect} ({'xyz' if xyz else 'mha'}, {mode}): extend the list"


def test_unfixed_dq_tail_gives_nan_only_with_strongly_negative_lse():
    """The defect the dQ kernel had: keys past Nk of the last tile unmasked.  Harmless at unit scores (p finite times a zero K row), NaN once
    lse < -88.7 (p = exp2(-lse2) = inf, inf * 0 in the second product)."""
    for regime, expect_nan in (("unit", False), ("shift_pos", False), ("shift_neg", True)):
        idx = next(i for i, c in enumerate(CASES) if c[0] == f"65x63-{regime}")
        for mode in ("fp32", "bf16"):
            inp = AR.make_inputs(CASES[idx][2], CASES[idx][3], regime, False, mode, H, seed=7)
            bad = AR.run(*inp[:4], CASES[idx][2], inp[4], mode, False, dq_no_tail_mask=True)
            assert bool(torch.isnan(bad["dq"][:, :65]).any()) == expect_nan, (regime, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("xyz", [False, True], ids=["mha", "xyz"])
def test_qzero_closed_form(xyz, mode):
    """q = 0: out = mean of V (xyz) over the Nk real keys, lse = log Nk, dK = 0 exactly, dV_j = sum_i dO_i / Nk, dQ = s sum_j (dO.(v_j - out)) k_j / Nk."""
    for idx, (name, kind, table, R, regime) in enumerate(CASES):
        if regime != "qzero":
            continue
        (q, k, v, go, scale), ref, got, err = _case(idx, xyz, mode)
        vh = v.double()[None].expand(H, -1, -1) if xyz else v.double()
        for (qs, nq, ks, nk) in table:
            mean = vh[:, ks:ks + nk].mean(1, keepdim=True)
            tol = AR.bound("o", mode, xyz, err, ref, table) * float(mean.abs().max())
            assert float((got["o"][:, qs:qs + nq].double() - mean).abs().max()) <= tol
            assert float((got["lse"][:, qs:qs + nq].double() - math.log(nk)).abs().max()) <= AR.bound("lse", mode, xyz, err, ref, table)
            assert float(got["dk"][:, ks:ks + nk].abs().max()) == 0.0
            assert float((ref["o"][:, qs:qs + nq] - mean).abs().max()) <= 1e-12 * max(1.0, float(mean.abs().max()))
            dO = go[:, qs:qs + nq].double()
            ds = (dO @ (vh[:, ks:ks + nk] - mean).transpose(1, 2)) / nk
            dq = scale * ds @ k[:, ks:ks + nk].double()
            assert float((ref["dq"][:, qs:qs + nq] - dq).abs().max()) <= 1e-12 * max(1.0, float(dq.abs().max()))
            if not xyz:
                dv = dO.sum(1, keepdim=True).expand(-1, nk, -1) / nk
                assert float((ref["dv"][:, ks:ks + nk] - dv).abs().max()) <= 1e-12 * max(1.0, float(dv.abs().max()))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_peaked_closed_form(mode):
    """One key leads every row by ~40: the xyz output IS that key's coordinates (~1e3) to fp32 rounding in both operand modes (coordinates
    never pass through bf16), and every gradient vanishes (p = 1 exactly, dS = dO.(x - out) = 0)."""
    for idx, (name, kind, table, R, regime) in enumerate(CASES):
        if not regime.startswith("peaked"):
            continue
        (q, k, v, go, scale), ref, got, err = _case(idx, True, mode)
        for prob in table:
            qs, nq, ks, nk = prob
            x = v[AR.peaked_key(prob, regime)]
            assert float(x.abs().max()) > 10.0
            assert float((got["o"][:, qs:qs + nq] - x).abs().max()) <= 2.0 ** -23 * float(x.abs().max())
            for nm in ("dq", "dk"):
                r0, n = AR.rows_of(nm, prob)
                assert float(got[nm][:, r0:r0 + n].abs().max()) <= peaked_grad_bound(scale, q, k, v, go)


def peaked_grad_bound(scale, q, k, v, go):
    """|dS| <= a few roundings of dO.(x - out) at the size |dO| |x|; dQ, dK = scale * dS * (one row of K / Q)."""
    return 16 * 2.0 ** -23 * 3 * float(go.abs().max()) * float(v.abs().max()) * scale * max(float(q.abs().max()), float(k.abs().max()))


def test_problem_table_rejects_empty_segments():
    from dreg_nerf_amd import attn_ops as A
    for segs in ([(0, 5)], [(5, 0)], [(4, 4), (3, 0)], [(4, 4), (-1, 2)]):
        with pytest.raises(ValueError):
            A.ProblemTable(segs, "cpu")
    t = A.ProblemTable([(3, 5), (2, 1)], "cpu")
    sp, cp, R = AR.segs_tables([(3, 5), (2, 1)])
    assert t.R == R and t.self_probs.tolist() == [list(p) for p in sp] and t.cross_probs.tolist() == [list(p) for p in cp] and t.max_len == 5
