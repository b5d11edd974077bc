"""GPU: the fused marching-cubes kernels (csrc/marching_cubes.hip, dreg_nerf_amd.mesh; rule: DESIGN.md §3h) against the CPU restatement
(tests/mc_restatement.py, itself held to table-free invariants by tests/test_mc_host.py).

* (b) all 256 configurations in one lattice, inside values in {1, 3}, outside 0, dyadic origin and spacing.  At level 0.75 every operation of the
  vertex rule is exact (t is 0.25 or 0.75) and verts and faces equal the fp64 restatement bit for bit.  At level 0.5 an edge whose inside end is 3
  has t = 1/6 or 5/6, which no binary format holds: there faces and V are exact, verts equal the fp32 same-order restatement bit for bit, equal
  the fp64 restatement bit for bit on every vertex whose inside end is 1, and stay within the counted rounding bound on the others.
* (c) seeded integer lattices at nx in {2, 3, 63, 64, 65, 129} x ny, nz in {2, 3, 5, 9} and one shape with 4,160 (y, z) rows, more than one scan
  block of 4,096: faces and V exact, verts bit for bit against the fp32 restatement and within mc_cases.vertex_bound of fp64.
* (d) a surface cut by the lattice boundary; (e) empty inputs; (f) identical bytes between runs; (g) every C guard; (h) block_mesh on a generated
  block; (i) the two entry points on a small split on disk."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import mc_cases as MC
import mc_restatement as M
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import mesh, ngp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
DYADIC = ((-2.0, 0.5, 1.0), (0.25, 0.5, 0.125))


def _run(values, level, origin, spacing):
    v, f = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(values)).to(DEV), level, origin, spacing)
    return v.cpu().numpy(), f.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------- (b)
def test_all_configurations_exact_at_level_075():
    values = MC.all_configs_lattice(0)
    verts, faces = _run(values, 0.75, *DYADIC)
    rv, rf = M.marching_cubes(values, 0.75, *DYADIC)
    assert faces.dtype == np.int32 and np.array_equal(faces, rf)
    assert np.array_equal(verts.astype(np.float64), rv), "every operation is exact here: fp32 on the device must equal fp64"
    assert M.is_closed(faces) and len(verts) == M.straddling_edge_count(values, 0.75)


def test_all_configurations_at_level_05():
    values = MC.all_configs_lattice(0)
    verts, faces = _run(values, 0.5, *DYADIC)
    rv, rf = M.marching_cubes(values, 0.5, *DYADIC)
    r32, _ = M.marching_cubes(values, 0.5, *DYADIC, fp32=True)
    assert np.array_equal(faces, rf) and verts.shape == rv.shape
    assert np.array_equal(_bits(verts), _bits(r32))
    # vertices of edges whose inside end is 1: t = 0.5, exact
    g = (rv - np.array(DYADIC[0])) / np.array(DYADIC[1])
    frac = np.abs(g - np.round(g)).max(axis=1)
    exact = np.isclose(frac, 0.5, atol=1e-12)
    assert 0 < exact.sum() < len(rv)
    assert np.array_equal(verts[exact].astype(np.float64), rv[exact])
    err = np.abs(verts.astype(np.float64) - rv).max(axis=0)
    bound = MC.vertex_bound((64, 64, 4), *DYADIC)
    print("level 0.5: max |fp32 - fp64| per axis", err, "bound", bound)
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------------------------- (c)
def _check_integer_lattice(nx, ny, nz, seed):
    values = MC.integer_lattice(nx, ny, nz, seed)
    verts, faces = _run(values, MC.LEVEL, MC.ORIGIN, MC.SPACING)
    rv, rf = M.marching_cubes(values, MC.LEVEL, MC.ORIGIN, MC.SPACING)
    r32, _ = M.marching_cubes(values, MC.LEVEL, MC.ORIGIN, MC.SPACING, fp32=True)
    tag = f"nx {nx} ny {ny} nz {nz}"
    assert verts.shape[0] == rv.shape[0] == M.straddling_edge_count(values, MC.LEVEL), tag
    assert np.array_equal(faces, rf), tag
    assert np.array_equal(_bits(verts), _bits(r32)), tag
    if len(rv):
        assert (np.abs(verts.astype(np.float64) - rv).max(axis=0) <= MC.vertex_bound((nx, ny, nz), MC.ORIGIN, MC.SPACING)).all(), tag
    return len(rv), len(rf)


@pytest.mark.parametrize("nx", MC.NX)
def test_integer_lattices_at_tile_edges(nx):
    total = [0, 0]
    for ny in MC.NYZ:
        for nz in MC.NYZ:
            v, f = _check_integer_lattice(nx, ny, nz, seed=7)
            total[0] += v
            total[1] += f
    assert total[0] > 0 and total[1] > 0


def test_integer_lattice_longer_than_one_scan_block():
    nx, ny, nz = MC.SCAN_SHAPE
    assert ny * nz > 4096
    v, f = _check_integer_lattice(nx, ny, nz, seed=11)
    assert v > 4096 and f > 4096


# ------------------------------------------------------------------------------------------------------------------- (d)
def test_surface_cut_by_the_lattice_boundary():
    values = MC.cut_lattice()
    nz, ny, nx = values.shape
    verts, faces = _run(values, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    rv, rf = M.marching_cubes(values, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), fp32=True)
    assert np.array_equal(faces, rf) and np.array_equal(_bits(verts), _bits(rv))
    d = M.directed_edge_counts(faces)
    assert max(d.values()) == 1
    once = [(a, b) for (a, b) in d if (b, a) not in d]
    assert len(once) > 0 and len(once) < len(d) // 4
    hi = np.array([nx - 1, ny - 1, nz - 1], dtype=np.float32)
    for a, b in once:                                        # an edge used once lies in a boundary face of the lattice: both ends on the SAME face
        on_a = np.concatenate([verts[a] == 0.0, verts[a] == hi])
        on_b = np.concatenate([verts[b] == 0.0, verts[b] == hi])
        assert (on_a & on_b).any(), (verts[a], verts[b])


# ------------------------------------------------------------------------------------------------------------------- (e)
def test_empty_and_degenerate_inputs():
    unit = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for values, level in ((np.zeros((5, 9, 70), np.float32), 0.5), (np.ones((5, 9, 70), np.float32), 0.5), (np.full((3, 3, 3), 2.0, np.float32), 2.0),
                          (np.full((3, 3, 3), np.nan, np.float32), 0.5), (np.ones((3, 3, 3), np.float32), float("nan"))):
        verts, faces = _run(values, level, *unit)
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and verts.dtype == np.float32 and faces.dtype == np.int32
    values = np.full((6, 9, 66), 2.0, dtype=np.float32)
    values[1, 2, 1] = values[4, 8, 65] = values[2, 3, 63] = values[2, 3, 64] = np.nan        # an inner node, a corner node, a pair across the wave's edge
    values[3, 5, 30] = np.inf
    values[3, 5, 31] = -np.inf
    verts, faces = _run(values, 1.0, *unit)
    rv, rf = M.marching_cubes(values, 1.0, *unit, fp32=True)
    assert len(rv) == 6 + 4 + 10 + 6 == M.straddling_edge_count(values, 1.0) and np.array_equal(faces, rf) and np.array_equal(_bits(verts), _bits(rv))


# ------------------------------------------------------------------------------------------------------------------- (f)
def test_two_runs_give_identical_bytes():
    values = torch.from_numpy(MC.integer_lattice(129, 9, 9, 3)).to(DEV)
    a = mesh.marching_cubes(values, MC.LEVEL, MC.ORIGIN, MC.SPACING)
    b = mesh.marching_cubes(values, MC.LEVEL, MC.ORIGIN, MC.SPACING)
    assert a[0].shape[0] > 0 and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------- (g)
def test_every_guard_returns_einval_without_a_launch():
    lib = L.load()
    nx, ny, nz = 5, 4, 3
    values = torch.from_numpy(MC.integer_lattice(nx, ny, nz, 0)).to(DEV)
    nb = int(lib.dreg_mc_workspace_bytes(nx, ny, nz))
    assert 0 < nb <= 8 * nx * ny * nz + 64
    assert lib.dreg_mc_workspace_bytes(1, 4, 4) == 0 and lib.dreg_mc_workspace_bytes(4, 1025, 4) == 0 and lib.dreg_mc_workspace_bytes(1024, 1024, 257) == 0
    assert 0 < lib.dreg_mc_workspace_bytes(1024, 1024, 256) <= 8 * 2 ** 28 + (1 << 16)
    SENT = -77
    ws = torch.full((nb // 4,), SENT, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), SENT, dtype=torch.int32, device=DEV)
    s = L.stream()
    count = lambda v, x, y, z, w, wb, c: lib.dreg_mc_count(v, x, y, z, 1.5, w, wb, c, s)
    P = L.ptr
    bad = [count(None, nx, ny, nz, P(ws), nb, P(counts)), count(P(values), nx, ny, nz, None, nb, P(counts)), count(P(values), nx, ny, nz, P(ws), nb, None),
           count(P(values), 1, ny, nz, P(ws), nb, P(counts)), count(P(values), nx, 1, nz, P(ws), nb, P(counts)), count(P(values), nx, ny, 1, P(ws), nb, P(counts)),
           count(P(values), 1025, ny, nz, P(ws), 1 << 40, P(counts)), count(P(values), nx, 1025, nz, P(ws), 1 << 40, P(counts)),
           count(P(values), nx, ny, 1025, P(ws), 1 << 40, P(counts)), count(P(values), 1024, 1024, 257, P(ws), 1 << 40, P(counts)),
           count(P(values), nx, ny, nz, P(ws), nb - 1, P(counts))]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((ws == SENT).all()) and bool((counts == SENT).all()), "a refused call wrote to the device"
    assert count(P(values), nx, ny, nz, P(ws), nb, P(counts)) == 0
    V, F = counts.tolist()
    assert V > 0 and F > 0
    verts = torch.full((V, 3), float(SENT), dtype=torch.float32, device=DEV)
    faces = torch.full((F, 3), SENT, dtype=torch.int32, device=DEV)
    org, spc = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)

    def emit(v=P(values), x=nx, y=ny, z=nz, level=1.5, o=org, sp=spc, w=P(ws), wb=nb, ve=P(verts), fa=P(faces), nv=V, nf=F):
        return lib.dreg_mc_emit(v, x, y, z, level, o, sp, w, wb, ve, fa, nv, nf, s)
    bad = [emit(v=None), emit(o=None), emit(sp=None), emit(w=None), emit(ve=None), emit(fa=None), emit(x=1), emit(y=1025), emit(wb=nb - 1),
           emit(nv=V - 1), emit(nv=V + 1), emit(nf=F - 1), emit(nf=F + 1), emit(nv=-1), emit(level=2.5), emit(x=ny, y=nx)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert bool((verts == SENT).all()) and bool((faces == SENT).all()), "a refused emit wrote to the device"
    assert emit() == 0
    torch.cuda.synchronize()
    rv, rf = M.marching_cubes(values.cpu().numpy(), 1.5, (0, 0, 0), (1, 1, 1), fp32=True)
    assert np.array_equal(faces.cpu().numpy(), rf) and np.array_equal(_bits(verts.cpu().numpy()), _bits(rv))
    w = ctypes.c_int(0)
    assert lib.dreg_mc_table(None, None) == -1 and lib.dreg_mc_table(None, ctypes.byref(w)) == 0 and w.value == M.load_table()[1]
    for shape in ((4, 4), (1, 4, 4)):
        with pytest.raises(ValueError):
            mesh.marching_cubes(torch.zeros(shape, device=DEV), 0.5)
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(4, 4, 4, device=DEV, dtype=torch.float64), 0.5)


# ------------------------------------------------------------------------------------------------------------------- (h)
def _field(seed=3):
    """The generated block of tests/test_hip_render.py: random hash grid and MLPs."""
    g = torch.Generator().manual_seed(seed)
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params[:3072] = torch.randn(3072, generator=g) * 1.0
        f.mlp_base.params[3072:] = torch.randn(f.mlp_base.params.numel() - 3072, generator=g)
        f.color_mlp.params.copy_(torch.randn(7168, generator=g) * 0.2)
    return f


def test_block_mesh_on_a_generated_block():
    field = _field().to(DEV).eval()
    res = 32
    m = mesh.block_mesh(field, res)
    verts, faces = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    assert m["level"] == 0.7 and len(verts) > 100 and len(faces) > 100
    assert M.is_closed(faces) and M.repeated_index_faces(faces) == 0
    # every vertex's edge, with the node densities re-queried through query_density, straddles the level
    n = res + 1
    axes = [torch.tensor(m["origin"][c], dtype=torch.float32) + torch.arange(n, dtype=torch.float32) * torch.tensor(m["spacing"][c], dtype=torch.float32) for c in range(3)]
    for c in range(3):
        assert float(axes[c][0]) == AABB[c]
        axes[c][-1] = AABB[3 + c]                            # the last node is queried ON the aabb face
    Z, Y, X = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    dens = field.query_density(torch.stack([X, Y, Z], dim=-1).reshape(-1, 3).to(DEV)).reshape(n, n, n).cpu().numpy()
    shell = np.ones_like(dens, dtype=bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert (dens[shell] == 0.0).all() and (dens[~shell] > 0.7).any() and (dens[~shell] <= 0.7).any()
    assert len(verts) == M.straddling_edge_count(dens, 0.7)
    assert M.vertices_on_straddling_edges(verts, dens, 0.7, m["origin"], m["spacing"])
    rv, rf = M.marching_cubes(dens, 0.7, m["origin"], m["spacing"], fp32=True)
    assert np.array_equal(faces, rf) and np.array_equal(_bits(verts), _bits(rv))
    # winding: the geometric normal of a face against the mean of its vertices' field normals (a sign check for a flipped table, not a tolerance)
    nrm, col = m["normals"].cpu().numpy().astype(np.float64), m["colors"].cpu().numpy()
    assert nrm.shape == verts.shape and col.shape == verts.shape and col.min() >= 0.0 and col.max() <= 1.0
    v64 = verts.astype(np.float64)
    geo = np.cross(v64[faces[:, 1]] - v64[faces[:, 0]], v64[faces[:, 2]] - v64[faces[:, 0]])
    dot = (geo * nrm[faces].mean(axis=1)).sum(axis=1)
    share = float((dot > 0).mean())
    area, vol = mesh.mesh_area_volume(m["verts"], m["faces"])
    print(f"block_mesh resolution {res}: V {len(verts)} F {len(faces)} area {area:.3f} volume {vol:.3f}; faces whose normal agrees with the field normals: {share:.4f}")
    assert share > 0.5
    assert vol > 0 and vol == pytest.approx(M.signed_volume(verts, faces), rel=1e-9)
    bare = mesh.block_mesh(field, res, normals=False, colors=False)
    assert bare["normals"] is None and bare["colors"] is None and torch.equal(bare["faces"], m["faces"])
    field.unbounded = True
    try:
        with pytest.raises(NotImplementedError):
            mesh.block_mesh(field, res)
    finally:
        field.unbounded = False


def test_block_mesh_winding_on_a_coarse_field():
    """The generated block's hash grid is noise at a 33^3 lattice's scale (the share above sits near one half).  The same block with only its
    three coarsest hash-grid levels (resolution 16 to about 30 cells) varies at the lattice's scale: there the sign of the winding shows.
    The level is the median density of the inner nodes, so the surface exists whatever the weights give."""
    field = _field()
    offsets = list(field._levels[0])
    with torch.no_grad():
        field.mlp_base.params[3072 + 2 * int(offsets[3]):] = 0.0
    field = field.to(DEV).eval()
    res = 32
    values = mesh.sample_density_lattice(field, res)
    level = float(values[1:-1, 1:-1, 1:-1].median())
    assert level > 0.0
    m = mesh.block_mesh(field, res, level=level, colors=False)
    verts, faces = m["verts"].cpu().numpy().astype(np.float64), m["faces"].cpu().numpy()
    assert len(faces) > 100 and M.is_closed(faces)
    geo = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    share = float(((geo * m["normals"].cpu().numpy().astype(np.float64)[faces].mean(axis=1)).sum(axis=1) > 0).mean())
    print(f"coarse field, level {level:.4f}: V {len(verts)} F {len(faces)}; faces whose normal agrees with the field normals: {share:.4f}")
    assert share > 0.5


# ------------------------------------------------------------------------------------------------------------------- (i)
def _write_block(path, seed, res=64):
    f = _field(seed)
    c = (torch.arange(res, dtype=torch.float32) + 0.5) / res * 3 - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    rad = torch.stack([X, Y, Z], -1).norm(dim=-1)
    occ = ngp.OccupancyGrid(AABB, res)
    occ._binary.copy_((rad > 0.55) & (rad < 1.05))
    cams = torch.eye(4)[None].repeat(6, 1, 1)
    cams[:, :3, 3] = torch.tensor([[2.5, 0, 0], [-2.5, 0, 0], [0, 2.5, 0], [0, -2.5, 0], [0, 0, 2.5], [0, 0, -2.5]])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"step": 1, "model": f.state_dict(), "occupancy_grid": occ.state_dict(), "aabb": AABB, "unbounded": False, "near_plane": None, "far_plane": None,
                "grid_resolution": res, "contraction_type": ngp.ContractionType.AABB, "render_step_size": 0.005, "alpha_thre": 0.0, "cone_angle": 0.0,
                "camera_poses": cams, "block_id": 0}, path)


def _main(monkeypatch, module, argv):
    import importlib
    import random
    monkeypatch.setattr(sys, "argv", [module + ".py"] + argv)
    monkeypatch.syspath_prepend(ROOT)
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(DEV))     # main() seeds the process: put it back
    try:
        importlib.import_module(module).main()
    finally:
        random.setstate(state[0])
        np.random.set_state(state[1])
        torch.set_rng_state(state[2])
        torch.cuda.set_rng_state(state[3], DEV)


def test_entry_points_write_the_meshes(tmp_path, monkeypatch, capsys):
    """eval_ngp_nerf.py --mesh and eval_nerf_regtr.py --merged_mesh (their main(), in this process) on a one-scene split of two generated blocks."""
    from dreg_nerf_amd import vis_dump
    root, res = str(tmp_path), 24
    a = np.deg2rad(20.0)
    T1 = torch.tensor([[np.cos(a), -np.sin(a), 0.0, 0.1], [np.sin(a), np.cos(a), 0.0, -0.05], [0.0, 0.0, 1.0, 0.02], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32)
    transforms = {0: torch.eye(4), 1: T1}
    os.makedirs(os.path.join(root, "objaverse", "images", "sceneA"))
    json.dump({str(k): v.tolist() for k, v in transforms.items()}, open(os.path.join(root, "objaverse", "images", "sceneA", "world_frame_transforms.json"), "w"))
    jd = os.path.join(root, "json")
    os.makedirs(jd)
    json.dump({"train": [], "test": ["sceneA"]}, open(os.path.join(jd, "objaverse.json"), "w"))
    ck = [os.path.join(root, "objaverse", "nerf_models", "sceneA", f"block_{k}", "model.pth") for k in (0, 1)]
    for k, p in enumerate(ck):
        _write_block(p, seed=5 + k)
    common = ["--root_dir", root, "--dataset", "objaverse", "--mesh_resolution", str(res)]
    _main(monkeypatch, "eval_ngp_nerf", common)                       # the extraction: the grids the registration reads
    before = {p: os.path.getmtime(os.path.join(os.path.dirname(p), "voxel_grid.pt")) for p in ck}
    _main(monkeypatch, "eval_ngp_nerf", common + ["--mesh"])
    out = capsys.readouterr().out
    assert out.count("mesh.ply") == 2 and " V " in out and " F " in out and "area" in out and "volume" in out
    from dreg_nerf_amd.visibility import load_block
    own = {}
    for p in ck:
        assert os.path.getmtime(os.path.join(os.path.dirname(p), "voxel_grid.pt")) == before[p]           # --mesh runs instead of the extraction
        v, f, c, nrm = vis_dump.read_mesh_ply(os.path.join(os.path.dirname(p), "mesh.ply"))
        m = mesh.block_mesh(load_block(p, DEV)[0], res)
        assert len(v) == m["verts"].shape[0] > 0 and len(f) == m["faces"].shape[0] > 0 and c.shape == v.shape and nrm.shape == v.shape
        assert np.array_equal(v, m["verts"].cpu().numpy().astype(np.float64)) and np.array_equal(f, m["faces"].cpu().numpy()) and M.is_closed(f)
        own[p] = m
    _main(monkeypatch, "eval_nerf_regtr", common + ["--json_dir", jd, "--expname", "t", "--merged_mesh"])
    d = os.path.join(root, "eval", "t", "objaverse", "sceneA")
    metrics = json.load(open(os.path.join(root, "eval", "t", "objaverse", "metrics_test.json")))
    assert set(metrics) == {"sceneA", "R_mean", "t_mean"} and set(metrics["sceneA"]) == {"R_mean", "t_mean", "R_med", "t_med", "time"}
    gt = vis_dump.read_mesh_ply(os.path.join(d, "merged_mesh_gt.ply"))
    pred = vis_dump.read_mesh_ply(os.path.join(d, "merged_mesh_pred.ply"))
    # which block was the source is the dataset's draw (quirk Q15): the gt file tells — its source half is one block's mesh moved by that order's pose
    matched = False
    for s, t in ((0, 1), (1, 0)):
        ms, mt = own[ck[s]], own[ck[t]]
        ns, nfs = ms["verts"].shape[0], ms["faces"].shape[0]
        if len(gt[0]) != ns + mt["verts"].shape[0]:
            continue
        P = transforms[t] @ torch.linalg.inv(transforms[s])
        moved, moved_n = mesh.transform_mesh(ms["verts"], ms["normals"], P.to(DEV))
        if not np.allclose(gt[0][:ns], moved.cpu().numpy().astype(np.float64), atol=1e-5):
            continue
        matched = True
        assert np.allclose(gt[3][:ns], moved_n.cpu().numpy(), atol=1e-5)
        for got in (gt, pred):
            assert len(got[0]) == ns + mt["verts"].shape[0] and len(got[1]) == nfs + mt["faces"].shape[0]
            assert np.array_equal(got[1][:nfs], ms["faces"].cpu().numpy()) and np.array_equal(got[1][nfs:], mt["faces"].cpu().numpy() + ns)
            assert np.array_equal(got[0][ns:], mt["verts"].cpu().numpy().astype(np.float64))
            assert M.is_closed(got[1])
        # the predicted file's source half is the same mesh under a rigid motion: edge lengths are kept
        e = ms["faces"].cpu().numpy()[:, :2]
        l0 = np.linalg.norm(ms["verts"].cpu().numpy()[e[:, 0]].astype(np.float64) - ms["verts"].cpu().numpy()[e[:, 1]], axis=1)
        l1 = np.linalg.norm(pred[0][e[:, 0]] - pred[0][e[:, 1]], axis=1)
        assert np.allclose(l0, l1, atol=1e-4)
    assert matched, "merged_mesh_gt.ply's source half is neither block's mesh moved by the known pose"
