"""CPU: the fp64 march restatement (tests/march_restatement.py) against hand counts and against the fp32 restatement of the renderer's rule
(tests/render_restatement.py), and the input sets of tests/test_hip_march_exact.py (tests/march_cases.py) against the conditions that make
that test mean something: at most 2 % of the rays (points) of a random or grazing set are undecidable, no ray ends early (n a <= 2), n can be
decoded from the opacity, and one misplaced sample moves the depth by at least four times the depth tolerance."""
import numpy as np
import pytest
import torch

import march_cases as C
import march_restatement as MR
import render_restatement as RR

CUBE = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
BIG = [-4.0, -4.0, -4.0, 4.0, 4.0, 4.0]
DT = 1.0 / 64
UNDECIDABLE_CAP = 0.02


def _march(binary, o, d, **kw):
    kw.setdefault("model", BIG)
    return MR.march(np.array([o], np.float32), np.array([d], np.float32), binary, CUBE, CUBE, kw.pop("model"), DT, exact=True, **kw)


def _single(i, j, k):
    b = np.zeros((8, 8, 8), bool)
    b[i, j, k] = True
    return b


FULL = np.ones((8, 8, 8), bool)


@pytest.mark.parametrize("o, d, hit, count, first", [
    ((-1.5, -0.9375, -0.9375), (1, 0, 0), True, 128, 0),          # outside: t_min = 0.5, 2 / dt samples
    ((-1.0, -0.9375, -0.9375), (1, 0, 0), True, 128, 0),          # on the face
    ((0.0, -0.9375, -0.9375), (1, 0, 0), True, 64, 0),            # inside
    ((0.0, -0.9375, -0.9375), (-1, 0, -0.0), True, 64, 0),
    ((-1.5, -1.0, -1.0), (1, 0, 0), True, 128, 0),                # in two boundary planes of the slab: o[k] == lo is a hit
    ((-1.5, 1.0, 1.0), (1, -0.0, 0), True, 128, 0),               # ... and o[k] == hi (u == 1: the last cell, by the clamp)
    ((-1.5, -0.9375, -0.9375), (-1, 0, 0), False, 0, None),       # pointing away
    ((-1.5, -1.5, 0.0), (1, 0, 0), False, 0, None),               # parallel to the slab, outside it
    ((1.0, 0.125, 0.125), (0, 1, 0), True, 56, 0),                # inside the +x face plane, from y = 0.125 to 1
    ((-1.0, -1.0, 0.125), (1, 1, 0), True, 128, 0),               # along a face diagonal: t runs 0 .. 2
    ((1.5, 0.0, 0.0), (1, 1, 0), False, 0, None),
])
def test_hand_counts_in_a_full_grid(o, d, hit, count, first):
    m = _march(FULL, o, d)
    assert bool(m.hit[0]) == hit and m.n_kept[0] == count and m.n_model[0] == count
    if count:
        n, t, _ = m.kept(0)
        assert n[0] == first and np.array_equal(n, np.arange(count)) and t[0] == m.t_min[0] + 0.5 * DT


def test_samples_on_cell_faces_belong_to_the_upper_cell():
    b = _single(4, 4, 4)                                           # the cell [0, 0.25)^3
    m = _march(b, (-0.5, 0.125, 0.125), (1, 0, 0), near_plane=1.0 / 128)     # x = -0.5 + (n + 1) / 64: x = 0 at n = 31, x = 0.25 at n = 47
    assert np.array_equal(m.kept(0)[0], np.arange(31, 47))
    m = _march(b, (0.5, 0.125, 0.125), (-1, 0, 0), near_plane=1.0 / 128)     # x = 0.5 - (n + 1) / 64: x = 0.25 at n = 15 (cell 5), x = 0 at n = 31
    assert np.array_equal(m.kept(0)[0], np.arange(16, 32))
    m = _march(b, (-0.5, 0.125, 0.125), (1, 0, 0))                            # midpoints: x = -0.5 + (2 n + 1) / 128, never on a face
    assert np.array_equal(m.kept(0)[0], np.arange(32, 48))


def test_planes_jitter_and_model_aabb():
    m = _march(FULL, (-1.5, 0.125, 0.125), (1, 0, 0), near_plane=0.5, far_plane=0.25)
    assert m.hit[0] and m.n_kept[0] == 0                           # near beyond far: the aabb is hit, the interval is empty
    m = _march(FULL, (-1.5, 0.125, 0.125), (1, 0, 0), near_plane=1.0, far_plane=1.5)
    assert m.n_kept[0] == 32 and m.kept(0)[1][0] == 1.0 + DT / 2
    m = _march(FULL, (-1.5, 0.125, 0.125), (1, 0, 0), jitter=np.array([0.5], np.float32))
    assert m.n_kept[0] == 127 and m.kept(0)[1][0] == 0.5 + DT      # t = 0.5 + (n + 1) dt < 2.5
    m = _march(FULL, (-1.5, 0.125, 0.125), (1, 0, 0), model=[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5])
    assert m.n_kept[0] == 128 and m.n_model[0] == 64               # outside the model aabb: kept, sigma = 0
    n, _, inm = m.kept(0)
    assert np.array_equal(n[inm], np.arange(32, 96))
    a = 0.25
    op, dep = m.composite(a)
    assert abs(op[0] - (1 - 0.75 ** 64)) < 1e-12
    assert abs(dep[0] - sum(a * 0.75 ** j * (0.5 + (32 + j + 0.5) * DT) for j in range(64))) < 1e-12


def test_ragged_last_cells_and_roi_inside_scene():
    b = np.zeros((8, 4, 16), bool)
    b[7, 3, 15] = True
    roi = [-1.0, -0.5, -2.0, 1.0, 0.5, 2.0]
    scene = [-2.0, -1.0, -4.0, 2.0, 1.0, 4.0]
    m = MR.march(np.array([[0.875, 0.375, -5.0]], np.float32), np.array([[0, 0, 1.0]], np.float32), b, roi, scene, BIG, DT, exact=True)
    # enters the scene at z = -4 (t = 1), the roi at z = -2, the cell [1.75, 2) at n = (5.75 - 1) * 64 = 368
    assert m.t_min[0] == 1.0 and np.array_equal(m.kept(0)[0], np.arange(368, 384))


def test_visibility_form():
    b = _single(4, 4, 4)
    cams = np.array([[-2.0, 0.125, 0.125]], np.float32)
    pts = np.array([[0.125, 0.125, 0.125], [-0.125, 0.125, 0.125], [-2.0, 0.125, 0.125], [0.0, 0.125, 0.125]], np.float32)
    lab, dec, m = MR.visibility(cams, pts, b, CUBE, CUBE, BIG, DT)
    # x = -1 + (2 n + 1) / 128 in [0, 0.125): n = 64 .. 71; the point in front of the cell sees nothing; t_max = 0 is no ray at all
    assert lab.tolist() == [True, False, False, False] and m.n_kept.tolist() == [8, 0, 0, 0]
    assert not m.hit[2] and m.t_max[0] == 2.125
    # OR over cameras: a second camera behind the cell sees the point in front of it
    lab2, _, _ = MR.visibility(np.array([[-2.0, 0.125, 0.125], [2.0, 0.125, 0.125]], np.float32), pts, b, CUBE, CUBE, BIG, DT)
    assert lab2.tolist() == [True, True, True, True]


def test_margin_flags_a_sample_next_to_an_occupied_face():
    b = _single(4, 4, 4)
    o = np.array([[-0.5, 0.125, 0.125]], np.float32)
    d = np.array([[1.0, 0.0, 0.0]], np.float32)
    assert not MR.march(o, d, b, CUBE, CUBE, BIG, DT, near_plane=1.0 / 128, far_plane=1.0 + 1.0 / 256).decidable[0]         # a sample exactly on the cell's face
    assert MR.march(o, d, b, CUBE, CUBE, BIG, DT).decidable[0]                                    # midpoints: 1/128 from every face
    assert MR.march(o, d, np.zeros((8, 8, 8), bool), CUBE, CUBE, BIG, DT, near_plane=1.0 / 128, far_plane=1.0 + 1.0 / 256).decidable[0]     # same occupancy on both sides
    assert not MR.march(o, d, b, CUBE, CUBE, [-4, -4, -4, 0.125 - 1.0 / 128, 4, 4], DT).decidable[0]              # a kept sample on the model's face
    assert not MR.march(o, d, b, CUBE, CUBE, BIG, DT, far_plane=0.5 + 1.0 / 128).decidable[0]                     # t_max on a lattice point


@pytest.mark.parametrize("grid", C.RANDOM_GRIDS)
@pytest.mark.parametrize("dt", C.RANDOM_DTS[:2])
def test_fp64_march_agrees_with_the_fp32_restatement_on_decidable_rays(grid, dt):
    c = C.random_case(grid, dt)
    r = c.ref
    tm, occ = RR.march(torch.from_numpy(c.o), torch.from_numpy(c.d), torch.from_numpy(c.binary), torch.tensor(c.roi), torch.tensor(c.scene), c.dt)
    S = max(occ.shape[1], int(r.n_idx.max()) + 1)
    mine = np.zeros((len(c.o), S), bool)
    mine[r.ray, r.n_idx] = True
    theirs = np.zeros_like(mine)
    theirs[:, :occ.shape[1]] = occ.numpy()
    same = (mine == theirs).all(axis=1)
    assert same[r.decidable].all(), np.nonzero(~same & r.decidable)[0][:10]
    assert r.decidable.mean() > 0.98 and r.n_kept.sum() > 10000


@pytest.mark.parametrize("grid", ["ragged", "random10"])
def test_fp32_stepping_agrees_with_the_fp64_march_on_decidable_rays(grid):
    """Case.stepped_fp32 (the rule in fp32 at every lattice point, what the GPU test holds the grazing rays at dt = 1e-3 against) keeps the
    fp64 samples wherever no rounding can change them — which also says that the margins of march_restatement cover real fp32 roundings."""
    c = C.random_case(grid, 0.005)
    r = c.ref
    kept, model = c.stepped_fp32()
    ok = (kept == r.n_kept) & (model == r.n_model)
    assert ok[r.decidable].all(), np.nonzero(~ok & r.decidable)[0][:10]


def _check_set(c):
    r = c.ref
    a = C.alpha64(c.dt)
    und = float((~r.decidable).mean())
    print(f"{c.name}: undecidable {und:.4f}, max n {int(r.n_model.max())}, depth tolerance {c.depth_tolerance():.3e}, "
          f"smallest one-step change of depth {c.step_sensitivity()[r.decidable].min():.3e}")
    assert und <= UNDECIDABLE_CAP, und
    n = r.n_model.max()
    assert n * a <= 2.0                                              # transmittance >= e^-2: far above the 1e-4 early stop
    assert n * 2.0 ** -24 / a <= 0.1                                 # decoding n from the opacity: n roundings of 2^-24 in units of a
    assert (c.step_sensitivity()[r.decidable] >= 4 * c.depth_tolerance()).all()
    return r


@pytest.mark.parametrize("grid", C.RANDOM_GRIDS)
@pytest.mark.parametrize("dt", C.RANDOM_DTS)
def test_random_input_sets(grid, dt):
    c = C.random_case(grid, dt)
    r = _check_set(c)
    for k, name in enumerate(C.FAMILIES):                            # every family marches something, within its own cap
        f = c.family == k
        assert (~r.decidable[f]).mean() <= UNDECIDABLE_CAP, name
        assert (r.n_kept[f & r.decidable] > 0).mean() > 0.2, name
    if grid != "shell128":
        assert (r.n_kept - r.n_model)[r.decidable].sum() > 1000      # samples outside the model aabb: kept and counted, sigma = 0
    graz = c.family == 1
    small = np.sort(np.abs(c.d[graz]), axis=1)[:, :2]
    assert small.max() < 2e-3 and (small < 1e-4).mean() > 0.3        # nearly axis-parallel: two components of order 1e-3 and smaller


@pytest.mark.parametrize("jitter", C.JITTERS, ids=[str(j) for j in C.JITTERS])
def test_training_input_sets(jitter):
    c = C.train_case(jitter)
    _check_set(c)
    assert c.jitter.max() < 1.0 and c.jitter.min() >= 0.0


@pytest.mark.parametrize("grid", sorted(C.EXACT_GRIDS))
@pytest.mark.parametrize("planes", sorted(C.EXACT_PLANES))
def test_exact_input_sets(grid, planes):
    """Every value is dyadic with few bits: fp32 evaluates the rule without rounding, so no ray is excluded.  The sets still have to contain the
    edge cases they are there for."""
    for pattern in C.EXACT_PATTERNS:
        c = C.exact_case(grid, planes, pattern)
        r = c.ref
        assert r.decidable.all()
        for arr in (c.o, c.d):
            assert np.array_equal(arr * 256, np.round(arr * 256))
        a = C.alpha64(c.dt)
        assert r.n_model.max() * a <= 2.0
        assert (c.step_sensitivity() >= 4 * c.depth_tolerance()).all()
    c = C.exact_case(grid, planes, "full")
    r = c.ref
    lo, hi = np.array(c.roi[:3]), np.array(c.roi[3:])
    assert r.hit.any() and (~r.hit).any()
    assert np.signbit(c.d[c.d == 0]).any() and (~np.signbit(c.d[c.d == 0])).any()
    on_face = ((c.o == lo) | (c.o == hi)).any(axis=1)
    in_plane = (((c.o == lo) | (c.o == hi)) & (c.d == 0)).any(axis=1)
    inside = ((c.o > lo) & (c.o < hi)).all(axis=1)
    outside = ((c.o < lo) | (c.o > hi)).any(axis=1)
    if planes == "near_beyond_far":
        assert r.n_kept.sum() == 0
    else:
        for mask in (on_face, in_plane, inside, outside):
            assert (r.n_kept[mask] > 0).any()
        assert (outside & ~r.hit).any()
    if planes == "faces":                                            # lattice points exactly on cell faces
        x = c.o[r.ray].astype(np.float64) + r.t_mid[:, None] * c.d[r.ray]
        assert (np.mod((x - lo) / ((hi - lo) / np.array(c.binary.shape)), 1.0) == 0).any()


def test_calibration_ray_keeps_one_sample():
    r = C.calibration_case().ref
    assert r.n_kept.tolist() == [1] and r.n_model.tolist() == [1]


@pytest.mark.parametrize("distinct", [True, False])
def test_visibility_input_sets(distinct):
    v = C.vis_case(distinct)
    lab, dec, m = v.ref
    print(f"{v.name}: undecidable points {(~dec).mean():.4f}")
    assert (~dec).mean() <= UNDECIDABLE_CAP
    assert 0.1 < lab.mean() < 0.9
    Nc, Np = len(v.cams), len(v.pts)
    diff = np.tile(v.pts, (Nc, 1)) - np.repeat(v.cams, Np, axis=0)
    zero = (diff == 0).sum(axis=1)
    assert (zero == 1).sum() > 100 and (zero == 2).sum() > 10 and (zero == 3).sum() >= 1        # axis-parallel rays, and t_max = 0 (a camera ON a point)
    assert (m.n_kept[zero >= 1] > 0).any()
    scene = np.array(v.scene)
    on_face = ((v.cams == np.float32(scene[:3])) | (v.cams == np.float32(scene[3:]))).any(axis=1)
    inside = ((v.cams > scene[:3]) & (v.cams < scene[3:])).all(axis=1)
    assert on_face.any() and inside.any() and (~on_face & ~inside).any()
