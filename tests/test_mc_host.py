"""CPU: the marching-cubes rule before any kernel runs.  The restatement (tests/mc_restatement.py) reads the derived triangle
table through dreg_mc_table, a host function of the library, and its meshes are held to table-free invariants: every directed edge occurs once
and its reverse once (closed, two triangles per edge), no face repeats an index, one vertex per straddling lattice edge, every vertex on such an
edge, positive signed volume (normals point to the lower values).  Checked for each of the 256 configurations on its own, for EVERY pairing of
neighbouring configurations along each axis (the 2^12 sign patterns of two cells that share a face), and on seeded random lattices; Euler
characteristic of a sphere and a torus; the mesh PLY writer; the committed table header against its generator; the new flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mc_cases as MC
import mc_restatement as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _check_closed_mesh(values, level, origin=UNIT[0], spacing=UNIT[1]):
    verts, faces = M.marching_cubes(values, level, origin, spacing)
    assert M.unmatched_edges(faces) == []
    assert M.repeated_index_faces(faces) == 0
    assert len(verts) == M.straddling_edge_count(values, level)
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < len(verts))
    assert M.vertices_on_straddling_edges(verts, values, level, origin, spacing)
    if (np.asarray(values) > level).any():
        assert M.signed_volume(verts, faces) > 0
    else:
        assert len(verts) == 0 and len(faces) == 0
    return verts, faces


def test_table_shape():
    tris, width = M.load_table()
    assert tris.shape == (256, 3 * width) and tris.dtype == np.int8 and tris.min() == -1 and tris.max() == 11
    assert not (tris[0] >= 0).any() and not (tris[255] >= 0).any()
    for row in tris:                                         # a row is whole triangles, then -1 to the end
        k = int((row >= 0).sum())
        assert k % 3 == 0 and (row[:k] >= 0).all() and (row[k:] == -1).all()
    assert max(int((r >= 0).sum()) // 3 for r in tris) == width


@pytest.mark.parametrize("inside", [1.0, 3.0])
def test_every_configuration_alone_is_closed_and_outward(inside):
    for cfg in range(256):
        _check_closed_mesh(MC.config_lattice(cfg, inside), 0.5)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_every_pairing_of_neighbouring_configurations(axis):
    values = MC.neighbour_pairs_lattice(axis)
    _check_closed_mesh(values, 0.5)


def test_random_shell_lattices():
    for seed in range(24):
        _check_closed_mesh(MC.random_shell_lattice(seed, density=(0.3, 0.5, 0.7)[seed % 3]), 0.5)


def test_fp32_mode_matches_fp64_on_exact_inputs_and_stays_within_the_bound_elsewhere():
    v = MC.all_configs_lattice(0)
    a, fa = M.marching_cubes(v, 0.75, (-2.0, 0.5, 1.0), (0.25, 0.5, 0.125))
    b, fb = M.marching_cubes(v, 0.75, (-2.0, 0.5, 1.0), (0.25, 0.5, 0.125), fp32=True)
    assert b.dtype == np.float32 and np.array_equal(fa, fb) and np.array_equal(a, b.astype(np.float64))
    v = MC.integer_lattice(65, 9, 5, 0)
    a, fa = M.marching_cubes(v, MC.LEVEL, MC.ORIGIN, MC.SPACING)
    b, fb = M.marching_cubes(v, MC.LEVEL, MC.ORIGIN, MC.SPACING, fp32=True)
    err = np.abs(a - b.astype(np.float64)).max(axis=0)
    assert np.array_equal(fa, fb) and (err <= MC.vertex_bound((65, 9, 5), MC.ORIGIN, MC.SPACING)).all() and err.max() > 0


def test_sphere_and_torus_euler_characteristic():
    v, o, s = MC.sphere_lattice(17)
    verts, faces = _check_closed_mesh(v, 0.0, o, s)
    assert M.euler_characteristic(len(verts), faces) == 2
    vol = M.signed_volume(verts, faces)
    assert 0.9 * 4 / 3 * np.pi * 0.7 ** 3 < vol < 4 / 3 * np.pi * 0.7 ** 3       # inscribed polyhedron of a convex body
    v, o, s = MC.torus_lattice(25)
    verts, faces = _check_closed_mesh(v, 0.0, o, s)
    assert M.euler_characteristic(len(verts), faces) == 0


def test_nan_counts_as_outside_and_equal_ends_make_no_vertex():
    v = np.full((4, 4, 4), 2.0, dtype=np.float32)
    assert M.marching_cubes(v, 1.0, *UNIT)[0].shape[0] == 0             # equal ends above the level
    assert M.marching_cubes(v, 2.0, *UNIT)[0].shape[0] == 0             # equal ends AT the level: value > level is false on both
    v[1, 2, 1] = np.nan
    verts, faces = M.marching_cubes(v, 1.0, *UNIT)
    assert len(verts) == 6 and len(faces) == 8 and M.is_closed(faces)    # an octahedron around the NaN node, every t = 0.5
    assert M.signed_volume(verts, faces) < 0                              # the OUTSIDE is enclosed: normals point at the NaN node
    assert np.array_equal(np.sort(np.abs(verts - np.array([1.0, 2.0, 1.0])).sum(axis=1)), np.full(6, 0.5))


def test_mesh_ply_round_trip(tmp_path):
    from dreg_nerf_amd import vis_dump
    v, o, s = MC.sphere_lattice(9)
    verts, faces = M.marching_cubes(v, 0.0, o, s)
    rng = np.random.default_rng(0)
    rgb, nrm = rng.random((len(verts), 3)), rng.standard_normal((len(verts), 3))
    for kw in (dict(), dict(rgb=rgb), dict(normals=nrm), dict(rgb=rgb, normals=nrm)):
        p = str(tmp_path / "m.ply")
        vis_dump.write_mesh_ply(p, verts, faces, **kw)
        rv, rf, rc, rn = vis_dump.read_mesh_ply(p)
        assert np.array_equal(rv, verts) and np.array_equal(rf, faces) and rf.dtype == np.int32
        assert (rc is None) == ("rgb" not in kw) and (rn is None) == ("normals" not in kw)
        if rc is not None:
            assert np.array_equal(rc, np.clip(np.round(rgb * 255.0), 0, 255).astype(np.uint8))
        if rn is not None:
            assert np.array_equal(rn, nrm)
        head = open(p, "rb").read(400).split(b"end_header\n")[0].decode("ascii")
        assert head.startswith("ply\nformat binary_little_endian 1.0\n") and f"element face {len(faces)}\nproperty list uchar int vertex_indices" in head
    # the vertex element is write_ply's, byte for byte
    vis_dump.write_ply(str(tmp_path / "pts.ply"), verts, rgb, nrm)
    pts = open(tmp_path / "pts.ply", "rb").read().split(b"end_header\n", 1)[1]
    mesh = open(p, "rb").read().split(b"end_header\n", 1)[1]
    assert mesh[:len(pts)] == pts and len(mesh) == len(pts) + 13 * len(faces)
    # an empty mesh is a valid file
    vis_dump.write_mesh_ply(p, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32))
    rv, rf, _, _ = vis_dump.read_mesh_ply(p)
    assert rv.shape == (0, 3) and rf.shape == (0, 3)


def test_committed_table_header_is_what_the_generator_writes(tmp_path):
    out = tmp_path / "mc_table.h"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_mc_table.py"), "--out", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(os.path.join(ROOT, "dreg_nerf_amd", "csrc", "mc_table.h"), "rb").read()


def test_mesh_flags_parse():
    from dreg_nerf_amd.config import config_parser
    cfg = config_parser([])
    assert cfg.mesh is False and cfg.merged_mesh is False and cfg.mesh_resolution == 256 and cfg.mesh_level is None
    cfg = config_parser(["--mesh", "--mesh_resolution", "64", "--mesh_level", "120.4", "--merged_mesh"])
    assert cfg.mesh and cfg.merged_mesh and cfg.mesh_resolution == 64 and cfg.mesh_level == 120.4


def test_mesh_helpers_on_the_host():
    """transform_mesh / merge_meshes / mesh_area_volume are plain torch: a unit-cube-like octahedron moved by a pose keeps area and volume."""
    import torch
    from dreg_nerf_amd import mesh
    v = np.full((5, 5, 5), 0.0, dtype=np.float32)
    v[2, 2, 2] = 1.0
    verts, faces = M.marching_cubes(v, 0.5, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    tv, tf = torch.from_numpy(verts).float(), torch.from_numpy(faces)
    area, vol = mesh.mesh_area_volume(tv, tf)
    assert vol == pytest.approx(M.signed_volume(verts, faces)) and vol == pytest.approx(1.0 / 6.0) and area == pytest.approx(8 * np.sqrt(3) / 8)
    P = torch.tensor([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25]])
    nrm = torch.nn.functional.normalize(tv - tv.mean(0), dim=1)
    mv, mn = mesh.transform_mesh(tv, nrm, P)
    assert torch.allclose(mv, tv @ P[:, :3].T + P[:, 3]) and torch.allclose(mn, nrm @ P[:, :3].T)
    a2, v2 = mesh.mesh_area_volume(mv, tf)
    assert a2 == pytest.approx(area) and v2 == pytest.approx(vol)
    both = mesh.merge_meshes({"verts": mv, "faces": tf, "normals": mn, "colors": None}, {"verts": tv, "faces": tf, "normals": nrm, "colors": None})
    assert both["verts"].shape[0] == 12 and torch.equal(both["faces"][len(tf):], tf + 6) and both["colors"] is None and both["normals"].shape == (12, 3)
    assert mesh.level_for_alpha(0.7, 1e-2) == pytest.approx(120.397, abs=1e-3) and mesh.DENSITY_THRE == 0.7
    with pytest.raises(ValueError, match="GPU"):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)
