"""CPU: the host side of the scene density field (dreg_nerf_amd/scene_field.py) — the lattice a scene is meshed on, the identities of
the fp64 restatement (tests/scene_field_restatement.py) the GPU tests lean on, the per-vertex blend on hand-made parts, and the evaluator's flag."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

import pair_field_restatement as PF
import scene_field_restatement as SF
from dreg_nerf_amd import pair_field as P
from dreg_nerf_amd import scene_field as S
from dreg_nerf_amd.config import config_parser

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose(deg=25.0, t=(-0.13, 0.02, 0.02), axis=2):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    R = {2: [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], 0: [[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], 1: [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]}[axis]
    M = np.eye(4)
    M[:3, :3] = np.array(R)
    M[:3, 3] = t
    return M


def _union_box(aabbs, poses):
    los, his = [], []
    for aabb, pose in zip(aabbs, poses):
        s = np.asarray(aabb, dtype=np.float64)
        corners = np.array([[s[3 * i], s[3 * j + 1], s[3 * k + 2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
        moved = corners if pose is None else corners @ np.asarray(pose)[:3, :3].T + np.asarray(pose)[:3, 3]
        los.append(moved.min(axis=0))
        his.append(moved.max(axis=0))
    return np.min(los, axis=0), np.max(his, axis=0)


# ------------------------------------------------------------------------------------------------------- scene_lattice
BOX_A, BOX_B, BOX_C = [-1.0, -0.5, -2.0, 1.0, 0.75, 0.5], [-0.3, -1.0, -1.0, 2.0, 1.0, 1.25], [100.0, 100.0, 100.0, 101.0, 103.0, 102.0]
CASES = [([AABB], [None], 16), ([BOX_A], [_pose(63.0, (10.0, -7.5, 3.25), axis=0)], 37),
         ([AABB, AABB], [_pose(), None], 24), ([BOX_A, BOX_B], [_pose(63.0, (10.0, -7.5, 3.25), axis=0), _pose(-12.0, (9.0, -7.0, 3.0), axis=1)], 50),
         ([AABB, AABB, AABB], [_pose(), _pose(-20.0, (-0.03, 0.018, 0.094), axis=0), None], 256),
         ([BOX_C, AABB, BOX_B], [_pose(-140.0, (0.1, 0.2, -0.3), axis=1)[:3], np.eye(4), _pose(5.0, (0.4, 0.0, 0.0))], 50),
         ([AABB, AABB, AABB, AABB], [_pose(), _pose(-20.0, (-0.03, 0.018, 0.094), axis=0), _pose(15.0, (-0.072, 0.011, 0.06), axis=1), _pose(0.0, (-0.222, 0.013, 0.087))], 24),
         ([BOX_A, BOX_B, BOX_A, AABB], [None, _pose(33.0, (0.5, 0.5, -0.25), axis=0), _pose(170.0, (-0.5, 0.0, 0.75), axis=1), None], 7)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_scene_lattice_margins_dimensions_and_fp32_exactness(case):
    aabbs, poses, res = CASES[case]
    origin, spacing, dims = S.scene_lattice(aabbs, [None if p is None else torch.from_numpy(np.asarray(p)) for p in poses], res)
    lo, hi = _union_box(aabbs, poses)
    ext = hi - lo
    h = ext.max() / res
    k_long = int(np.argmax(ext))
    for k in range(3):
        assert dims[k] == (res + 3 if k == k_long else math.ceil(ext[k] / h) + 3)
    assert all(float(np.float32(v)) == v for v in origin + spacing) and spacing[0] == spacing[1] == spacing[2]
    assert h <= spacing[0] <= h * (1 + 2.0 ** -19)
    # margins: the first and the last node of every axis lie at least one spacing outside the box of all aabbs (fp64 of the fp32 values is exact here)
    for k in range(3):
        first, last = origin[k], origin[k] + (dims[k] - 1) * spacing[k]
        assert lo[k] - first >= spacing[k] and last - hi[k] >= spacing[k], (k, lo[k] - first, last - hi[k], spacing[k])
        assert lo[k] - first <= 2.001 * spacing[k] + 2.0 ** -20 * abs(lo[k]) and last - hi[k] <= 2.001 * spacing[k] + 2.0 ** -20 * abs(hi[k])


def test_scene_lattice_of_a_pair_is_pair_lattice_exactly():
    for (s, t, pose, res) in [(AABB, AABB, _pose(), 16), (AABB, AABB, _pose(), 24), (AABB, AABB, _pose(), 256), (AABB, AABB, np.eye(4), 7),
                              (BOX_A, BOX_B, _pose(63.0, (10.0, -7.5, 3.25), axis=0), 37), (BOX_C, AABB, _pose(-140.0, (0.1, 0.2, -0.3), axis=1)[:3], 50)]:
        assert S.scene_lattice([s, t], [pose, None], res) == P.pair_lattice(s, t, pose, res)
    assert S.scene_lattice([AABB, AABB], [_pose(), None], 24)[2] == (27, 27, 22)
    assert S.scene_lattice([AABB], [None], 8)[2] == (11, 11, 11)


def test_scene_lattice_refuses_what_the_kernels_refuse():
    with pytest.raises(ValueError, match="dimension exceeds"):
        S.scene_lattice([AABB, AABB, AABB], [None, np.eye(4), None], 1022)
    with pytest.raises(ValueError, match="exceed 2\\^28"):
        S.scene_lattice([AABB, AABB, AABB], [None, np.eye(4), None], 700)
    flat = [-1.5, -1.5, -0.1, 1.5, 1.5, 0.1]
    assert S.scene_lattice([flat] * 3, [None, np.eye(4), None], 1021)[2] == (1024, 1024, 72)
    with pytest.raises(ValueError):
        S.scene_lattice([AABB], [None], 0)
    with pytest.raises(ValueError):
        S.scene_lattice([AABB], [np.eye(3)], 16)
    with pytest.raises(ValueError, match="span no volume"):
        S.scene_lattice([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], [None], 16)
    with pytest.raises(ValueError):
        S.scene_lattice([], [], 16)
    with pytest.raises(ValueError):
        S.scene_lattice([AABB] * 5, [None] * 5, 16)
    with pytest.raises(ValueError):
        S.scene_lattice([AABB] * 2, [None], 16)


# ------------------------------------------------------------------------------------------------------- the restatement's own identities
def _shell(seed, res, lo, hi):
    c = (np.arange(res) + 0.5) / res * 3 - 1.5
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    rad = np.sqrt(X * X + Y * Y + Z * Z)
    rng = np.random.default_rng(seed)
    return ((rad > lo) & (rad < hi)) & (rng.random((res, res, res)) > 0.1)


def _mk(seed, shell, center, k):
    return dict(roi=AABB, binary=_shell(seed, 24, *shell), center=center,
                sigma=lambda x: 5.0 * np.exp(-((x - 0.1 * k) ** 2).sum(axis=1)) + 0.3 * (1 + np.sin(3.0 * x[:, k % 3])))


BLOCKS = [_mk(1, (0.55, 1.05), [0.3, -2.2, 0.6], 1), _mk(2, (0.45, 0.95), [2.1, 0.4, 0.5], 2), _mk(3, (0.5, 1.0), [-1.8, 1.5, 0.7], 3),
          _mk(4, (0.6, 1.1), [0.5, 0.4, 2.3], 4)]
POSES = [_pose(), _pose(-20.0, (-0.03, 0.018, 0.094), axis=0), _pose(15.0, (-0.072, 0.011, 0.06), axis=1), None]


def _scene(K, order=None, seed=0, n=20000):
    order = list(range(K)) if order is None else order
    x = (np.random.default_rng(seed).random((n, 3)) * 2 - 1) * 1.2
    blocks = [BLOCKS[i] for i in order]
    poses = [POSES[i] if i < K - 1 else None for i in order]       # (the last block of a K-block scene takes the points as they are)
    return SF.scene_density(blocks, [SF.to_block(x, p) for p in poses]), x


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_restatement_weights_sum_to_one_where_any_block_covers_and_vanish_where_a_block_does_not(K):
    r, _ = _scene(K)
    m, om = r["m"], r["weight_block"]
    cnt = m.sum(axis=1)
    for c in range(K + 1):
        assert (cnt == c).sum() > 100, (K, c, int((cnt == c).sum()))
    assert np.abs(om[cnt > 0].sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -52
    assert (om[~m] == 0).all() and (om[m] > 0).all() and (om.sum(axis=1)[cnt == 0] == 0).all()
    alone = m & (cnt == 1)[:, None]
    assert (om[alone] == 1).all() and np.array_equal(r["sigma"][cnt == 1], r["sigma_block"][alone])
    assert (r["sigma"][cnt == 0] == 0).all() and (r["sigma_block"][~m] == 0).all()
    if K >= 2:
        shared = om[m & (cnt >= 2)[:, None]]
        assert ((shared > 0) & (shared < 1)).all()


@pytest.mark.parametrize("K", [2, 3, 4])
def test_restatement_permuting_the_blocks_permutes_the_weights_and_keeps_the_field(K):
    base, _ = _scene(K, seed=1)
    for order in itertools.permutations(range(K)):
        r, _ = _scene(K, list(order), seed=1)
        assert np.array_equal(r["m"], base["m"][:, list(order)])
        # 1 / (1 + 1/Q) against 1 - 1 / (1 + Q), and sums of <= 3 positive terms in another order: a few roundings of numbers <= 1
        assert np.abs(r["weight_block"] - base["weight_block"][:, list(order)]).max() <= 8 * 2.0 ** -52
        assert np.array_equal(r["sigma_block"], base["sigma_block"][:, list(order)])
        scale = np.maximum(base["sigma"], 1.0)
        assert (np.abs(r["sigma"] - base["sigma"]) <= 32 * 2.0 ** -52 * scale).all() and base["sigma"].max() > 1.0


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_restatement_coincident_identical_blocks_share_equally(K):
    x = (np.random.default_rng(2).random((10000, 3)) * 2 - 1) * 1.2
    r = SF.scene_density([BLOCKS[1]] * K, [x] * K)
    m = r["m"][:, 0]
    assert m.sum() > 1000 and (~m).sum() > 1000 and (r["m"] == m[:, None]).all()
    assert np.abs(r["weight_block"][m] - 1.0 / K).max() <= 2.0 ** -52 and (r["weight_block"][~m] == 0).all()
    own = np.where(m, BLOCKS[1]["sigma"](x), 0.0)
    assert (np.abs(r["sigma"] - own) <= 4 * 2.0 ** -52 * np.maximum(own, 1.0)).all()
    if K == 2:
        assert (r["weight_block"][m] == 0.5).all()


def test_restatement_of_two_blocks_is_the_pair_restatement():
    pose = _pose()
    x_t = (np.random.default_rng(0).random((20000, 3)) * 2 - 1) * 1.2
    x_s = SF.to_block(x_t, pose)
    assert np.array_equal(x_s, PF.to_source(x_t, pose))
    want = PF.pair_density(BLOCKS[0], BLOCKS[1], x_s, x_t)
    got = SF.scene_density(BLOCKS[:2], [x_s, x_t])
    assert (want["m_src"] & want["m_tgt"]).sum() > 2000
    assert np.array_equal(got["m"], np.stack([want["m_src"], want["m_tgt"]], axis=1))
    assert np.array_equal(got["weight_block"], np.stack([want["w_src"], want["w_tgt"]], axis=1))
    assert np.array_equal(got["sigma_block"], np.stack([want["sigma_src"], want["sigma_tgt"]], axis=1))
    assert np.array_equal(got["sigma"], want["sigma"])
    both = want["m_src"] & want["m_tgt"]
    y = PF.log_ratio(x_s, x_t, BLOCKS[0]["center"], BLOCKS[1]["center"])
    assert np.abs(SF.log_ratios(got["m"], got["delta"])[both] - np.abs(y[both])).max() <= 1e-14
    # the fp32 position: the pair restatement's, and the untouched point without a pose
    x32 = x_t.astype(np.float32)
    assert np.array_equal(SF.to_block_f32(x32, SF.pose_f32(pose)), PF.to_source_f32(x32, *PF.pose_f32(pose)))
    assert SF.to_block_f32(x32, SF.pose_f32(None)) is not None and np.array_equal(SF.to_block_f32(x32, None), x32)
    assert np.array_equal(SF.covered(AABB, BLOCKS[0]["binary"], x_s, fp32=True), PF.covered(AABB, BLOCKS[0]["binary"], x_s, fp32=True))


# ------------------------------------------------------------------------------------------------------- the per-vertex blend
def test_scene_attribute_blend_on_hand_made_rows():
    R90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])      # 90 degrees about z, exactly: x -> y, y -> -x
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    # rows: 0 one block (block 1, rotated) | 1 two shared | 2 three shared | 3 no block | 4 zero density | 5 cancelling gradients
    wb = f64([[0.0, 1.0, 0.0], [0.25, 0.0, 0.75], [0.5, 0.25, 0.25], [0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.5, 0.5, 0.0]])
    sb = f64([[9.0, 2.0, 9.0], [4.0, 7.0, 4.0], [2.0, 4.0, 4.0], [3.0, 3.0, 3.0], [0.0, 0.0, 5.0], [2.0, 2.0, 0.0]])
    g0 = f64([[5.0, 5, 5], [0.0, 4, 0], [0.0, 0, 2], [1.0, 2, 3], [0.0, 0, 0], [3.0, 0, 0]])
    g1 = f64([[2.0, 0, 0], [1.0, 1, 1], [0.0, 0, 4], [1.0, 2, 3], [0.0, 0, 0], [0.0, 3, 0]])
    g2 = f64([[7.0, 7, 7], [0.0, 4, 0], [0.0, 0, 4], [1.0, 2, 3], [9.0, 9, 9], [5.0, 5, 5]])
    cols = [f64([[0.9, 0.8, 0.7]] * 6), f64([[0.1, 0.2, 0.3]] * 6), f64([[0.5, 0.5, 0.1]] * 6)]
    Rs = [None, torch.from_numpy(R90), None]
    nrm, col, share = S.blend_scene_attributes(wb, sb, Rs, [g0, g1, g2], cols)
    # row 0: R (2,0,0) = (0,2,0); row 1: 0.25 (0,4,0) + 0.75 (0,4,0); row 2: 0.5 (0,0,2) + 0.25 (0,0,4) + 0.25 (0,0,4), a = (1, 1, 1)
    # row 5: 0.5 (3,0,0) + 0.5 R (0,3,0) = (1.5,0,0) + (-1.5,0,0)
    want_n = [[0, -1, 0], [0, -1, 0], [0, 0, -1], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    want_s = [[0, 1, 0], [0.25, 0, 0.75], [1 / 3, 1 / 3, 1 / 3], [0, 0, 0], [0, 0, 0], [0.5, 0.5, 0]]
    want_c = [[0.1, 0.2, 0.3], [0.6, 0.575, 0.25], [0.5, 0.5, 1.1 / 3], [0, 0, 0], [0, 0, 0], [0.5, 0.5, 0.5]]
    assert np.abs(nrm.numpy() - np.array(want_n, dtype=np.float64)).max() <= 1e-15
    assert np.abs(share.numpy() - np.array(want_s)).max() <= 1e-15 and np.abs(col.numpy() - np.array(want_c)).max() <= 1e-15
    assert torch.equal(col[0], cols[1][0])                                    # one carrier: its own colour, bit for bit
    assert (nrm[3:] == 0).all() and (col[3:5] == 0).all() and (share[3:5] == 0).all()
    rn, rc, rs = SF.vertex_attributes(wb.numpy(), sb.numpy(), [None, R90, None], [g0.numpy(), g1.numpy(), g2.numpy()], [c.numpy() for c in cols])
    assert np.abs(nrm.numpy() - rn).max() <= 1e-15 and np.abs(col.numpy() - rc).max() <= 1e-15 and np.abs(share.numpy() - rs).max() <= 1e-15
    assert S.blend_scene_attributes(wb, sb, Rs, [g0, g1, g2])[1] is None
    # one block alone: share 1, normal and colour its own
    n1, c1, s1 = S.blend_scene_attributes(f64([[1.0], [0.0]]), f64([[3.0], [3.0]]), [None], [f64([[0.0, 0, 2], [0.0, 0, 2]])], [f64([[0.3, 0.6, 0.9]] * 2)])
    assert torch.equal(n1, f64([[0.0, 0, -1], [0.0, 0, 0]])) and torch.equal(c1, f64([[0.3, 0.6, 0.9], [0.0, 0, 0]])) and torch.equal(s1, f64([[1.0], [0.0]]))


@pytest.mark.parametrize("K", [2, 3, 4])
def test_scene_attribute_blend_on_random_parts_against_the_restatement(K):
    g = torch.Generator().manual_seed(K)
    V = 500
    m = torch.rand(V, K, generator=g) > 0.4
    raw = torch.rand(V, K, generator=g) * m
    wb = raw / raw.sum(dim=1, keepdim=True).clamp(min=1e-30)
    sb = torch.rand(V, K, generator=g) * 50 * m
    grads = [torch.randn(V, 3, generator=g) * 30 for _ in range(K)]
    cols = [torch.rand(V, 3, generator=g) for _ in range(K)]
    Rn = [_pose(25.0 * (b + 1), axis=b % 3)[:3, :3] if b < K - 1 else None for b in range(K)]
    nrm, col, share = S.blend_scene_attributes(wb, sb, [None if R is None else torch.from_numpy(R).float() for R in Rn], grads, cols)
    rn, rc, rs = SF.vertex_attributes(wb.numpy(), sb.numpy(), Rn, [t.numpy() for t in grads], [c.numpy() for c in cols])
    assert nrm.dtype == torch.float32 and int((~m).all(dim=1).sum()) > 0 and int((m.sum(dim=1) == K).sum()) > 10
    # unit vectors and convex combinations of numbers in [0,1] from <= 10 + 4 K fp32 operations each; |g| is far from cancelling on random parts
    assert np.abs(nrm.numpy() - rn).max() <= 2e-5 and np.abs(col.numpy() - rc).max() <= 4e-6 and np.abs(share.numpy() - rs).max() <= 4e-6
    assert (col.numpy() >= 0).all() and (col.numpy() <= 1).all() and (share.numpy() >= 0).all() and (share.numpy() <= 1).all()
    tot = share.double().sum(dim=1)
    assert (((tot - 1).abs() <= K * 2.0 ** -23) | (tot == 0)).all()
    # a single carrier's colour is its own, bit for bit
    a = wb * sb
    for b in range(K):
        only = (a[:, b] != 0) & ((a != 0).sum(dim=1) == 1)
        assert int(only.sum()) > 0 and torch.equal(col[only], cols[b][only])


def test_scene_attribute_blend_of_two_blocks_is_the_pair_blend_bit_for_bit():
    g = torch.Generator().manual_seed(0)
    V = 2000
    w = torch.rand(V, generator=g)
    m_s, m_t = torch.rand(V, generator=g) > 0.3, torch.rand(V, generator=g) > 0.3
    ws = torch.where(m_s, torch.where(m_t, w, torch.ones(V)), torch.zeros(V))
    wt = torch.where(m_t, torch.where(m_s, 1 - w, torch.ones(V)), torch.zeros(V))
    ss, st = torch.rand(V, generator=g) * 50 * m_s, torch.rand(V, generator=g) * 50 * m_t
    ss[::7] = 0.0                                                            # zero densities under non-zero weights too
    gs, gt = torch.randn(V, 3, generator=g) * 30, torch.randn(V, 3, generator=g) * 30
    cs, ct = torch.rand(V, 3, generator=g), torch.rand(V, 3, generator=g)
    R = torch.from_numpy(_pose(25.0)[:3, :3]).float()
    bits = lambda t: t.contiguous().view(torch.int32)
    for colours in (True, False):
        want = P.blend_vertex_attributes(ws, wt, ss, st, R, gs, gt, cs if colours else None, ct if colours else None)
        got = S.blend_scene_attributes(torch.stack([ws, wt], dim=1), torch.stack([ss, st], dim=1), [R, None], [gs, gt], [cs, ct] if colours else None)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[2][:, 0]), bits(want[2]))
        assert (got[1] is None and want[1] is None) if not colours else torch.equal(bits(got[1]), bits(want[1]))
    assert int(((got[2][:, 0] > 0) & (got[2][:, 0] < 1)).sum()) > 200


def test_scene_attribute_blend_of_two_blocks_is_the_pair_blend_on_empty_and_nan_rows():
    """rows: 0 a_T = 0 | 1 a_S = 0 | 2 both a = 0 by the weights | 3 both a = 0 by the densities | 4 sigma_S NaN | 5 w_T NaN | 6 shared and finite;
    under a rotated source, with and without colours: the same bits from both functions, and zeros wherever the denominator is 0 or not a number."""
    nan = float("nan")
    ws, wt = torch.tensor([1.0, 0.0, 0.0, 0.5, 0.5, 0.5, 0.25]), torch.tensor([0.0, 1.0, 0.0, 0.5, 0.5, nan, 0.75])
    ss, st = torch.tensor([3.0, 9.0, 4.0, 0.0, nan, 2.0, 4.0]), torch.tensor([7.0, 2.0, 4.0, 0.0, 2.0, 2.0, 4.0])
    g = torch.Generator().manual_seed(1)
    gs, gt = torch.randn(7, 3, generator=g), torch.randn(7, 3, generator=g)
    cs, ct = torch.rand(7, 3, generator=g), torch.rand(7, 3, generator=g)
    R = torch.from_numpy(_pose(63.0, axis=0)[:3, :3]).float()
    bits = lambda t: t.contiguous().view(torch.int32)
    for colours in (False, True):
        want = P.blend_vertex_attributes(ws, wt, ss, st, R, gs, gt, cs if colours else None, ct if colours else None)
        got = S.blend_scene_attributes(torch.stack([ws, wt], dim=1), torch.stack([ss, st], dim=1), [R, None], [gs, gt], [cs, ct] if colours else None)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[2][:, 0]), bits(want[2]))
        assert (got[1] is None and want[1] is None) if not colours else torch.equal(bits(got[1]), bits(want[1]))
    assert torch.equal(want[2], torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.25])) and (got[2][2:6] == 0).all()
    assert torch.equal(got[1][0], cs[0]) and torch.equal(got[1][1], ct[1]) and (got[1][2:6] == 0).all() and (got[1][6] > 0).all()
    assert (got[0][2] == 0).all() and (got[0][5] == 0).all() and torch.isfinite(got[0]).all()


# ------------------------------------------------------------------------------------------------------- the evaluator's flag
def test_scene_mesh_field_flag_parses_and_implies_register_scene(monkeypatch):
    cfg = config_parser([])
    assert cfg.scene_mesh_field is False and cfg.register_scene is False and cfg.mesh_resolution == 256 and cfg.mesh_level is None
    cfg = config_parser(["--scene_mesh_field", "--mesh_resolution", "24", "--mesh_level", "1.5"])
    assert cfg.scene_mesh_field is True and cfg.register_scene is False and cfg.render_scene is False and cfg.merged_mesh_field is False
    assert cfg.mesh_resolution == 24 and cfg.mesh_level == 1.5
    monkeypatch.syspath_prepend(ROOT)
    import importlib
    ev = importlib.import_module("eval_nerf_regtr")
    cfg = ev.implied_flags(cfg)
    assert cfg.register_scene is True and cfg.scene_mesh_field is True and cfg.render_scene is False
    assert ev.implied_flags(config_parser(["--render_scene"])).register_scene is True
    plain = ev.implied_flags(config_parser(["--merged_mesh_field"]))
    assert plain.register_scene is False and plain.scene_mesh_field is False
