"""No GPU: the merged voxel grid of a registered scene (csrc/scene_grid.hip, dreg_nerf_amd/scene_grid.py; rule: DESIGN.md §3l).

* Known answers of the restatement (tests/scene_grid_restatement.py): two blocks with hand-set a and c, one carrier, an infinite a, no carrier,
  the fp32 sample position, alpha / keep, the zero rows.
* Every DREG_EINVAL guard of dreg_scene_voxel_grid, as tests/test_march_args_host.py tests the marchers': the device pointers are made-up
  addresses, so a guard that let a call through would launch on them and return a hipError_t (or fault) instead of DREG_EINVAL; the outputs'
  made-up addresses cannot have been written.  (tests/test_hip_scene_grid.py repeats the guards on real sentinel buffers.)
* scene_box against scene_lattice's box; the flag parses and implies --register_scene."""
import ctypes
import math

import numpy as np
import pytest

import scene_grid_restatement as SG
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import scene_field as S
from dreg_nerf_amd import scene_grid as G

EINVAL = -1
DEV = 0x10000                 # stands for a device buffer: the entry point reads through none of them on the host
_u16 = (ctypes.c_uint32 * 16)(*range(16))
_f16 = (ctypes.c_float * 16)(*[1.0] * 16)
_unit = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
_v3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
_pose = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0.2, 0.3)
A = ctypes.addressof


# ------------------------------------------------------------------------------------------------------- the restatement's known answers
def test_blend_of_two_blocks_with_hand_set_parts():
    a = np.array([[1.0, 3.0], [2.0, 0.0], [0.0, 5.0], [0.0, 0.0], [np.inf, 4.0], [np.inf, np.inf], [1e308, 1e308]])
    c = np.zeros((7, 2, 3))
    c[:, 0] = [0.2, 0.4, 0.8]
    c[:, 1] = [0.6, 0.0, 0.4]
    got = SG.blend(a, c)
    assert np.allclose(got[0], [(0.2 + 1.8) / 4, 0.4 / 4, (0.8 + 1.2) / 4], rtol=0, atol=1e-15)       # (a_0 c_0 + a_1 c_1) / (a_0 + a_1)
    assert np.array_equal(got[1], c[1, 0]) and np.array_equal(got[2], c[2, 1])                       # one carrier: its colour itself
    assert np.array_equal(got[3], np.zeros(3))                                                      # no carrier
    assert np.array_equal(got[4], c[4, 0])                                                          # an infinite a: the largest a's colour
    assert np.array_equal(got[5], c[5, 0])                                                          # a tie: the lowest index
    assert np.array_equal(got[6], c[6, 0]) and np.isfinite(got).all()                               # the denominator overflows
    a3 = np.array([[1.0, np.inf, np.inf], [0.0, 2.0, 2.0]])
    c3 = np.arange(18, dtype=np.float64).reshape(2, 3, 3) / 20
    got3 = SG.blend(a3, c3)
    assert np.array_equal(got3[0], c3[0, 1]) and np.allclose(got3[1], (c3[1, 1] + c3[1, 2]) / 2, rtol=0, atol=1e-15)


def test_sample_positions_alpha_keep_and_zero_rows():
    res, box = (2, 3, 4), [-1.0, 0.0, 2.0, 1.0, 3.0, 4.0]
    w = SG.sample_positions_f32(res, box)
    assert w.dtype == np.float32 and w.shape == (24, 3)
    x, y, z = SG.cell_indices(res)
    assert np.array_equal(x * 12 + y * 4 + z, np.arange(24)) and z[1] == 1 and y[4] == 1 and x[12] == 1      # z fastest
    assert np.array_equal(w[0], np.float32([-0.5, 0.5, 2.25])) and np.array_equal(w[23], np.float32([0.5, 2.5, 3.75]))
    j = np.full((24, 3), 0.25, dtype=np.float32)
    assert np.array_equal(SG.sample_positions_f32(res, box, j)[13], np.float32([(1.25 / 2) * 2 - 1, (0.25 / 3) * 3, (1.25 / 4) * 2 + 2]))
    # the fp32 expression, not its fp64 value rounded: a third is not exact
    u = (np.float32(1.0) + np.float32(0.25)) / np.float32(3.0)
    assert SG.sample_positions_f32((3, 3, 3), [0, 0, 0, 0.7, 0.7, 0.7], np.full((27, 3), 0.25, np.float32))[13, 0] == u * np.float32(0.7) + np.float32(0)
    alpha, keep = SG.alpha_keep(np.array([0.0, 0.7, 0.7000001, 50.0, np.inf, np.nan]))
    assert alpha[0] == 0 and alpha[3] == pytest.approx(1 - math.exp(-0.5)) and alpha[4] == 1.0
    assert keep.tolist() == [False, False, True, True, True, False]
    # one block, no pose: a ball of density 2 (kept) inside the block's grid; rows of unkept cells are exactly 0
    binary = np.ones((4, 4, 4), dtype=bool)
    blk = dict(roi=[-1, -1, -1, 1, 1, 1], binary=binary, center=[0, 0, 3.0], sigma=lambda p: np.where((p ** 2).sum(1) < 0.6, 2.0, 0.1),
               rgb=lambda p: np.tile([0.25, 0.5, 0.75], (len(p), 1)))
    out = SG.scene_grid([blk], [None], (6, 6, 6), [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5])
    keep = out["keep"]
    assert 0 < keep.sum() < keep.size and np.array_equal(out["voxel_mask"], np.nonzero(keep)[0])
    assert not out["voxel_grid"][~keep].any()
    rows = out["voxel_grid"][keep]
    assert np.array_equal(rows[:, :3], out["w"][keep].astype(np.float64)) and (rows[:, 3:6] == [0.25, 0.5, 0.75]).all()
    assert np.allclose(rows[:, 6], 1 - math.exp(-0.02), rtol=0, atol=1e-15)
    outside = (np.abs(out["w"]) > 1).any(axis=1)
    assert outside.any() and not out["sigma"][outside].any()                 # the block's own coverage ends at its roi


# ------------------------------------------------------------------------------------------------------- the C guards
def _blocks(n=3, over=None):
    """A HOST array of n dreg_radiance_block with made-up device pointers; over: {(block, field name): value}."""
    arr = (L.RadianceBlock * n)()
    for k in range(n):
        f = arr[k].field
        f.binary, f.rx, f.ry, f.rz = DEV, 8, 8, 8
        f.table = f.w1 = f.w2 = DEV
        f.offset = f.size = f.res = f.hashed = A(_u16)
        f.scale = A(_f16)
        f.roi_aabb = f.model_aabb = A(_unit)
        f.center = A(_v3)
        f.pose = A(_pose) if k == 0 else None
        arr[k].cw1 = arr[k].cw2 = arr[k].cw3 = arr[k].dirbias = DEV
    for (k, name), v in (over or {}).items():
        setattr(arr[k].field if name in dict(L.FieldBlock._fields_) else arr[k], name, v)
    return arr


def _call(res=(8, 8, 8), box=(0, 0, 0, 1, 1, 1), box_null=False, jitter=None, K=3, blocks="default", power=4.0, delta=1e-2, thre=0.7, grid=DEV, keep=DEV,
          sigma=None, over=None):
    arr = _blocks(max(K, 1) if 1 <= K <= 4 else 3, over) if blocks == "default" else blocks
    b = (ctypes.c_float * 6)(*box)
    return L.load().dreg_scene_voxel_grid(*res, None if box_null else A(b), jitter, K, None if arr is None else ctypes.cast(arr, ctypes.c_void_p), power, delta,
                                          thre, grid, keep, sigma, None)


NAN, INF = float("nan"), float("inf")
POINTERS = [n for n, _ in L.FieldBlock._fields_ if n not in ("rx", "ry", "rz", "pose")] + ["cw1", "cw2", "cw3", "dirbias"]
BAD = ([("null_aabb", dict(box_null=True)), ("null_blocks", dict(blocks=None)), ("null_grid", dict(grid=None)), ("null_keep", dict(keep=None))] +
       [(f"n_blocks_{K}", dict(K=K)) for K in (0, -1, 5)] +
       [(f"res_{'x'.join(str(v) for v in r)}", dict(res=r)) for r in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025), (1024, 1024, 257))] +
       [(f"box_{i}", dict(box=b)) for i, b in enumerate(((0, 0, 0, 0, 1, 1), (0, 0, 0, 1, -1, 1), (0, 0, 0, 1, 1, 0), (0, 0, 0, INF, 1, 1), (-INF, 0, 0, 1, 1, 1),
                                                         (0, NAN, 0, 1, 1, 1), (0, 0, 0, 1, 1, NAN), (-3e38, 0, 0, 3e38, 1, 1)))] +
       [(f"power_{p}", dict(power=p)) for p in (0.0, -1.0, NAN, INF)] + [(f"delta_{d}", dict(delta=d)) for d in (0.0, -1e-2, NAN, INF)] +
       [(f"thre_{t}", dict(thre=t)) for t in (NAN, INF, -INF)] +
       [(f"block{k}_null_{n}", dict(over={(k, n): None})) for k in range(3) for n in POINTERS] +
       [(f"block{k}_{n}_{v}", dict(over={(k, n): v})) for k, n, v in ((0, "rx", 0), (1, "ry", -1), (2, "rz", 0))])


def test_the_pointer_list_is_every_pointer_of_a_block_but_the_pose():
    assert len(POINTERS) == 16 and ctypes.sizeof(L.RadianceBlock) == ctypes.sizeof(L.FieldBlock) + 4 * ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("case", [c for c, _ in BAD])
def test_rejected_before_any_launch(case):
    assert _call(**dict(BAD)[case]) == EINVAL


# ------------------------------------------------------------------------------------------------------- the box, the flag
def _rot(axis, deg, t):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    P = np.eye(4)
    P[:3, :3] = {"z": [[c, -s, 0], [s, c, 0], [0, 0, 1]], "x": [[1, 0, 0], [0, c, -s], [0, s, c]]}[axis]
    P[:3, 3] = t
    return P


def test_scene_box_is_the_box_scene_lattice_spans():
    aabbs = [[-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], [-1.0, -2.0, -0.5, 1.0, 2.0, 0.5], [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]]
    poses = [_rot("z", 25.0, (-0.13, 0.02, 0.02)), _rot("x", -20.0, (0.4, 0.018, 0.094)), None]
    box = G.scene_box(aabbs, poses)
    assert G.scene_box is S.scene_box and len(box) == 6 and all(float(np.float32(v)) == v for v in box)
    # fp64 box from the corners, independently
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for ab, P in zip(aabbs, poses):
        cs = np.array([[ab[3 * i], ab[3 * j + 1], ab[3 * k + 2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
        if P is not None:
            cs = cs @ P[:3, :3].T + P[:3, 3]
        lo, hi = np.minimum(lo, cs.min(0)), np.maximum(hi, cs.max(0))
    for k in range(3):                                                       # rounded outward, by less than one fp32 step
        assert box[k] <= lo[k] and box[3 + k] >= hi[k]
        assert float(np.nextafter(np.float32(box[k]), np.float32(np.inf))) > lo[k] and float(np.nextafter(np.float32(box[3 + k]), np.float32(-np.inf))) < hi[k]
    ext = hi - lo
    assert not np.isclose(ext[0], ext[2])                                    # not made cubic
    # scene_lattice's lattice is spanned over the same box: h = longest extent / resolution, origin = lo - h
    for resolution in (16, 37):
        origin, spacing, dims = S.scene_lattice(aabbs, poses, resolution)
        h = ext.max() / resolution
        assert spacing[0] == S._f32_up(h * (1.0 + 2.0 ** -20)) and dims == tuple(resolution + 3 if k == int(np.argmax(ext)) else int(math.ceil(ext[k] / h)) + 3 for k in range(3))
        assert origin == [S._f32_down(float(lo[k]) - spacing[0]) for k in range(3)]
    assert G.scene_box(aabbs[:1], [None]) == aabbs[0]
    for bad in (([], []), (aabbs, poses[:2]), (aabbs * 2, poses * 2), ([[0, 0, 0, 0, 1, 1]], [None])):
        with pytest.raises(ValueError):
            G.scene_box(*bad)


def test_scene_voxel_grid_flag_parses_and_implies_register_scene(monkeypatch):
    import os
    monkeypatch.syspath_prepend(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from dreg_nerf_amd.config import config_parser
    import eval_nerf_regtr as E
    cfg = config_parser([])
    assert cfg.scene_voxel_grid is False and cfg.scene_grid_resolution == 128 and E.implied_flags(cfg).register_scene is False
    cfg = E.implied_flags(config_parser(["--scene_voxel_grid", "--scene_grid_resolution", "48"]))
    assert cfg.scene_voxel_grid is True and cfg.register_scene is True and cfg.scene_grid_resolution == 48 and cfg.scene_mesh_field is False and cfg.render_scene is False
