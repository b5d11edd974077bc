"""CPU: the fp64 restatement of the training backward (tests/render_bwd_restatement.py) against autograd on a general field, and the planted
field and input sets of tests/test_hip_render_bwd_fp64.py (tests/render_bwd_cases.py) against the conditions that make that test mean
something: the planted forward is exact, the early stop and the kept sets are decidable on all but 2 % of the rays, every level of the table
receives gradient, and each of fourteen deliberate errors of the restatement moves an element beyond four times the GPU test's bound."""
import functools

import numpy as np
import pytest
import torch

import march_cases as C
import march_restatement as MR
import render_bwd_cases as B
import render_bwd_restatement as RB
import render_train_restatement as RT
import test_hip_render_bwd_fp64 as G
from oracle import ngp_oracle as N

UNDECIDABLE_CAP = 0.02
DENSITIES = ("thin", "dense")


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def test_restatement_equals_autograd_on_a_general_field():
    """backward64, fed the oracle's own forward record of a random non-flat field, against autograd through render_train_restatement on that
    field: relative L2 <= 1e-4 per matrix and per table level (both sides are CPU references; the fp32 autograd side sets the figure)."""
    case = C.random_case("ragged", 0.02, "random")
    sel = np.arange(0, 4500, 30)
    o, d, jit = torch.from_numpy(case.o[sel]), torch.from_numpy(case.d[sel]), torch.from_numpy(case.jitter[sel])
    gen = torch.Generator().manual_seed(3)
    base = torch.empty(3072 + N.n_grid_params()).uniform_(-0.5, 0.5, generator=gen)
    base[:3072].uniform_(-0.3, 0.3, generator=gen)
    color = torch.empty(7168).uniform_(-0.3, 0.3, generator=gen)
    base.requires_grad_(True)
    color.requires_grad_(True)
    g_rgb = torch.randn(len(sel), 3, generator=gen)
    binary = torch.from_numpy(case.binary)
    rgb, _, _, surv = RT.render_train(base, color, case.model, o, d, binary, case.roi, case.scene, case.dt, jit, C.BKGD)
    (rgb * g_rgb).sum().backward()
    # the oracle's forward record of the same samples
    with torch.no_grad():
        roi, scene, model = (torch.tensor(v, dtype=torch.float32) for v in (case.roi, case.scene, case.model))
        tm, occ = RT.march(o, d, binary, roi, scene, case.dt, jit)
        idx = torch.nonzero(occ)
        x = o[idx[:, 0]] + tm[idx[:, 0], idx[:, 1], None] * d[idx[:, 0]]
        u = (x - model[:3]) / (model[3:] - model[:3])
        inm = ((u > 0) & (u < 1)).all(-1)
        w1, w2, table = N.split_density_params(base.detach())
        enc = N.hash_encode(u, N.f16(table))
        hd = N.f16(torch.relu(enc @ N.f16(w1).T))
        raw = N.f16(hd @ N.f16(w2).T)
        c1, c2, c3 = N.split_color_params(color.detach())
        xin = torch.cat([N.f16(N.sh4(d[idx[:, 0]])), raw[:, 1:16], torch.ones(len(idx), 1)], 1)
        h1 = N.f16(torch.relu(xin @ N.f16(c1).T))
        h2 = N.f16(torch.relu(h1 @ N.f16(c2).T))
        col = N.f16(torch.sigmoid(N.f16(h2 @ N.f16(c3).T)[:, :3]))
        assert torch.equal(col, N.query_rgb(d[idx[:, 0]], raw, color.detach()))
    ptr = np.concatenate([[0], np.cumsum(occ.sum(1).numpy())]).astype(np.int64)
    m = MR.Marched(ptr, idx[:, 1].numpy().astype(np.int64), tm[idx[:, 0], idx[:, 1]].double().numpy(), inm.numpy(), None, None, None, None, None)
    record = {k: v.double().numpy() for k, v in dict(enc=enc, hd=hd, raw=raw, xin=xin, h1=h1, h2=h2, c=col).items()}
    record["x"] = x.numpy()
    f16w = lambda t: N.f16(t).double().numpy()
    weights = dict(d1=f16w(w1), d2=f16w(w2), c1=f16w(c1), c2=f16w(c2), c3=f16w(c3))
    a = 1.0 - np.exp(-np.exp(record["raw"][:, 0] - 1.0) * case.dt)
    res = RB.backward64(record, weights, m, a, 1.0 - a, g_rgb.numpy(), C.BKGD, case.dt, B.levels(), case.model)
    assert np.array_equal(res.surv, surv.numpy()[idx[:, 0].numpy(), idx[:, 1].numpy()]) and res.surv.sum() > 1000
    assert (~m.in_model & res.surv).sum() > 50                        # survivors outside the model aabb exist
    gb, gc = base.grad.double().numpy(), color.grad.double().numpy()
    ref = {"d1": gb[:2048].reshape(64, 32), "d2": gb[2048:3072].reshape(16, 64), "c1": gc[:2048].reshape(64, 32),
           "c2": gc[2048:6144].reshape(64, 64), "c3": gc[6144:6144 + 192].reshape(3, 64)}
    # the reference's second form (sums, compositing and gradients in fp64 between the same fp16 roundings): its distance from the fp32 form
    b64, c64 = base.detach().clone().requires_grad_(True), color.detach().clone().requires_grad_(True)
    rgb64 = RT.render_train(b64, c64, case.model, o, d, binary, case.roi, case.scene, case.dt, jit, C.BKGD, dtype=torch.float64)[0]
    assert rgb64.dtype == torch.float64 and float((rgb64.detach() - rgb.detach()).abs().max()) < 2e-3
    (rgb64 * g_rgb.double()).sum().backward()
    gc64 = c64.grad.double().numpy()
    ref64 = {"c1": gc64[:2048].reshape(64, 32), "c2": gc64[2048:6144].reshape(64, 64), "c3": gc64[6144:6144 + 192].reshape(3, 64),
             "d1": b64.grad[:2048].double().numpy().reshape(64, 32), "d2": b64.grad[2048:3072].double().numpy().reshape(16, 64)}
    for k in RB.MATRICES:
        r, r64 = _rel(res.val[k], ref[k]), _rel(ref64[k], ref[k])
        print(f"restatement vs autograd, {k}: rel L2 {r:.3e}; fp64 form of the reference vs its fp32 form: {r64:.3e}")
        assert r <= 1e-4, (k, r)
        assert r64 <= 5e-3, (k, r64)                                   # (an fp16 rounding that falls the other way in a few activations)
    assert not gc[6144 + 192:].any()
    tab = gb[3072:]
    dense = np.zeros_like(tab)
    dense[res.t_idx] = res.t_val
    for l, row in enumerate(N.level_table()[0]):
        s = slice(2 * row["offset"], 2 * (row["offset"] + row["size"]))
        r = _rel(dense[s], tab[s])
        print(f"restatement vs autograd, table level {l}: rel L2 {r:.3e} over {int((tab[s] != 0).sum())} elements")
        assert r <= 1e-4, (l, r)


@pytest.mark.parametrize("which", ["model_is_scene", "model_inside_scene"])
def test_general_field_reference_holds_its_figures_block_by_block(which):
    """What the reference of tests/test_hip_ngp_train.py::test_backward_matches_cpu_autograd can hold on its own, on that test's very block
    and rays: the restatement run with an fp32 forward against the same with an fp64 forward (render_train(dtype=torch.float64)), both with
    the fp16 straight-through roundings, through the same blocks_of.  Four times the distance stays inside cosine >= 0.999 and relative L2
    <= 2e-2 for EVERY block, so that test gives no block a margin of its own.  (Between two forms of the reference; no kernel runs here.)"""
    import test_hip_ngp_train as T
    model = T.AABB if which == "model_is_scene" else T.MODEL_INSIDE
    f, g = T._block(torch.device("cpu"), seed=3)
    with torch.no_grad():
        f.aabb.copy_(torch.tensor(model, dtype=torch.float32))
    n, dt, bk = 300, 0.02, torch.ones(3)
    rays = T._rays(n, seed=4)
    jitter = torch.rand(n, generator=torch.Generator().manual_seed(5))
    g_rgb = torch.randn(n, 3, generator=torch.Generator().manual_seed(6)) / n
    mask = torch.ones(n)
    _, _, rb, rc, s32 = T._cpu_reference(f, g, rays, jitter, dt, bk, g_rgb, mask, model)
    touched = RT.reached_entries(mask.bool())
    _, _, rb64, rc64, s64 = T._cpu_reference(f, g, rays, jitter, dt, bk, g_rgb, mask, model, dtype=torch.float64)
    assert torch.equal(s32, s64)
    worst = (0.0, 0.0)
    for what, (sel, idx) in T.blocks_of(rb, rc, touched).items():
        cos, r = T.cos_rel((rb, rc)[sel][idx], (rb64, rc64)[sel][idx])
        print(f"REFDIST {which} {what}: cosine {cos:.8f}, rel L2 {r:.3e}")
        worst = (max(worst[0], 1.0 - cos), max(worst[1], r))
        assert 4 * (1.0 - cos) <= 1e-3 and 4 * r <= 2e-2, (what, cos, r)
    print(f"REFDIST {which}: largest 1 - cosine {worst[0]:.2e}, largest rel L2 {worst[1]:.3e}")


def test_planted_field_is_exact():
    for dens in DENSITIES:
        p = B.planted(dens)
        f = p["fwd"]
        for k in ("enc", "hd", "raw", "xin", "h1", "h2", "o"):
            assert np.array_equal(f[k].astype(np.float16).astype(np.float64), f[k]), k
        for k in ("hd", "h1", "h2"):
            pre = f[k + "_pre"]
            assert np.all((pre == 0) | (np.abs(pre) >= 1.0 / 64)) and 0.25 <= (pre > 0).mean() <= 0.75, k
        assert len(set(p["v"].ravel().tolist())) == 32 and np.all(p["v"] != 0) and np.array_equal(p["v"] * 16, np.round(p["v"] * 16))
        o = f["o"][:3]
        assert len(set(o.tolist())) == 3 and np.all(np.abs(o) <= 2)
        assert np.all(B.f16_boundary_distance(1.0 / (1.0 + np.exp(-o))) >= 8 * 2.0 ** -24)
        assert not p["weights"]["c1"][:, :16].any() and p["weights"]["c1"][:, 31].all()
        assert f["raw"][0] == B.H0[dens]
        # the oracle agrees: its encoding of the flat table is v at every point, faces and corners included, and its colour is c
        rng = np.random.default_rng(0)
        u = rng.random((2000, 3)).astype(np.float32)
        u[:300] = np.round(u[:300])
        u[300:600, 0] = 1.0
        base = torch.from_numpy(p["base"])
        enc = N.hash_encode(torch.from_numpy(u), N.f16(N.split_density_params(base)[2]))
        assert np.array_equal(enc.double().numpy(), np.broadcast_to(f["enc"], (2000, 32)))
        dens_o, raw = N.query_density(torch.from_numpy(u * 0.5 + 0.25), torch.tensor([0.0, 0, 0, 1, 1, 1]), base)
        assert np.array_equal(raw.double().numpy(), np.broadcast_to(f["raw"], (2000, 16)))
        col = N.query_rgb(torch.randn(2000, 3), raw, torch.from_numpy(p["color"]))
        assert np.array_equal(col.double().numpy(), np.broadcast_to(p["c"], (2000, 3)))


@pytest.mark.parametrize("dens", DENSITIES)
def test_early_stop_is_decidable(dens):
    """For every fp32 alpha within 4 * 2^-24 of the fp64 one (what the GPU test accepts from the kernel), q = fl32(1 - a): no q^n lies within
    n 2^-22 relative of the early-stop threshold, so n roundings of T *= q cannot change which sample is the last."""
    a64 = B.alpha64(B.H0[dens])
    a = np.float32(a64)
    cand = [a]
    for _ in range(70):
        cand += [np.nextafter(cand[-1], np.float32(1))]
    for _ in range(70):
        cand += [np.nextafter(min(cand), np.float32(0))]
    cand = [x for x in cand if abs(float(x) - a64) <= 4 * 2.0 ** -24]
    assert len(cand) >= 3
    worst = np.inf
    for x in cand:
        q = float(np.float32(1) - x)
        n = np.arange(1, 2000)
        gap = np.abs(q ** n / RB.EPS - 1.0) / (n * 2.0 ** -22)
        worst = min(worst, gap.min())
    print(f"{dens}: {len(cand)} candidate alphas, closest q^n to 1e-4 is {worst:.1f} x its margin n 2^-22")
    assert worst > 1.0


@functools.lru_cache(maxsize=None)
def _reference(name, dens, mutate=None):
    case = B.edge_set(int(name[4:])) if name.startswith("edge") else B.planted_set(C.JITTERS[int(name)])
    p = B.planted(dens)
    a = float(np.float32(B.alpha64(p["h0"])))
    q = float(np.float32(1) - np.float32(a))
    g = B.g_rgb_of(case) * (case.ref.decidable)[:, None]
    res = RB.backward64(B.record_of(p, case, case.ref), p["weights"], case.ref, a, q, g, B.BKGD, case.dt, B.levels(), case.model, mutate=mutate)
    return case, res


@pytest.mark.parametrize("j", range(len(C.JITTERS)), ids=[str(j) for j in C.JITTERS])
def test_planted_sets(j):
    """Undecidable rays (the march's, plus the early stop's) <= 2 % per set; every level receives gradient at >= 100 entries; a hashed level
    has an entry reached from two different cells; kept samples outside the model aabb exist; the dense field stops rays early."""
    for dens in DENSITIES:
        case, res = _reference(str(j), dens)
        r = case.ref
        und = float((~(r.decidable & res.firm)).mean())
        hits = int((r.n_kept > 0).sum())
        early = int((~res.surv).sum())
        per_level = np.bincount(res.t_level, minlength=16) // 2
        print(f"{case.name} {dens}: undecidable {und:.4f}, {hits} rays keep samples (max in-model {int(r.n_model.max())}), {int(res.surv.sum())} survivors, "
              f"{early} samples after the early stop, entries per level {per_level.tolist()}, entries reached from two cells {res.collisions}")
        assert und <= UNDECIDABLE_CAP and hits <= B.SET_RAYS and hits > 500
        assert per_level.min() >= 100
        lv = B.levels()
        assert any(res.collisions[l] > 0 for l in range(16) if lv["hashed"][l])
        assert (r.n_kept - r.n_model)[r.decidable].sum() > 100
        assert (early == 0) if dens == "thin" else (early > 1000)
    assert np.all(np.array(case.model[:3]) > np.array(case.roi[:3])) and np.all(np.array(case.model[3:]) < np.array(case.roi[3:]))


def test_edge_and_wide_sets():
    """The rays at the lane and chunk edges carry gradient: rays 0, 62, 63, 64, 127, 128 and n - 1 of every edge set, and every index of
    WIDE_HITS, are decidable and keep samples inside the model aabb; between them the sets keep misses and rays outside the model."""
    for n in B.EDGE_COUNTS:
        c = B.edge_set(n)
        assert len(c.o) == n and len(np.unique(np.concatenate([c.o, c.d], 1), axis=0)) == n
        for i in sorted({p for p in B.EDGE_LANES + (n - 1,) if p < n}):
            assert c.ref.decidable[i] and c.ref.n_model[i] >= 5, (n, i)
        if n >= 63:
            assert (c.ref.n_kept == 0).any() and ((c.ref.n_kept > 0) & (c.ref.n_model == 0)).any()
    w = B.wide_set()
    assert len(w.o) == B.WIDE_RAYS == 131072 + 1
    r = w.ref
    hitting = np.nonzero(r.hit)[0]
    assert set(hitting.tolist()) <= set(w.where.tolist()) and len(w.where) == B.SET_RAYS
    for i in B.WIDE_HITS:
        assert r.hit[i] and r.decidable[i] and r.n_model[i] >= 5, i
    src = B.planted_set("random")
    assert np.array_equal(np.sort(w.o[w.where], axis=0), np.sort(src.o, axis=0))          # the same rays as the 2,000-ray set, reordered
    m = B.miss_set()
    assert not m.ref.hit.any() and m.ref.hit_sure.all()


@pytest.mark.parametrize("mutate", RB.MUTATIONS)
def test_every_mutation_is_seen(mutate):
    """Each deliberate error of the restatement moves at least one element beyond 4 x the GPU test's bound (C + n) 2^-24 M, or moves an
    element that test requires to be exactly 0 (bound 0: an untouched table entry, a row of an inactive unit)."""
    best, zero_moved = 0.0, 0
    for name in ("edge129", "3"):
        for dens in DENSITIES:
            case, ref = _reference(name, dens)
            _, mut = _reference(name, dens, mutate)
            K = int(case.ref.n_model.max())
            bnd = G.bounds(ref, K, B.H0[dens])
            for k in RB.MATRICES:
                diff = np.abs(mut.val[k] - ref.val[k])
                live = bnd[k] > 0
                best = max(best, float((diff[live] / bnd[k][live]).max()))
                zero_moved += int((diff[~live] > 0).sum())
            dense = dict(zip(mut.t_idx.tolist(), mut.t_val.tolist()))
            got = np.array([dense.get(i, 0.0) for i in ref.t_idx.tolist()])
            best = max(best, float((np.abs(got - ref.t_val) / bnd["table"]).max()))
            zero_moved += int(np.setdiff1d(mut.t_idx[mut.t_val != 0], ref.t_idx).size)
            if best > 4.0 or zero_moved:
                break
        if best > 4.0 or zero_moved:
            break
    print(f"mutation {mutate}: largest |change| / bound = {best:.3g}; elements that must be exactly 0 and are not: {zero_moved}")
    assert best > 4.0 or zero_moved > 0
