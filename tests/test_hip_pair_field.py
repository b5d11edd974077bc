"""GPU: the pair density field (dreg_pair_density of csrc/scene_field.hip, dreg_nerf_amd/pair_field.py; rule: DESIGN.md §3i; restatement: tests/pair_field_restatement.py).

* The parts are the blocks' own dense queries bit for bit, masked by a torch statement of the coverage rule; the blend is exact given its parts.
* The overlap weight against the fp64 restatement on the shared points: |dw| <= 5e-6.  With y = 0.5 p ln q, |dw/dy| <= 1/4; taking the native
  exp2 / log2 within 2 ulp and adding the roundings of their argument scalings, |dy| <= |y| 2^-21 + 2^-20, so |dw| <= 6.3e-7 at |y| <= 2.3 (asserted);
  the bound is 8 times that.  The test prints the largest |dw| it saw (recorded in profiles/pair_field_accuracy.txt).
* The same block twice under the identity: w = 1/2 exactly, the field is the masked block, the mesh is the masked block's.
* One block empty: the lattice, the mesh and its attributes are the other block's.
* Lattice form == points form; permutations permute; two runs give identical bytes.
* pair_mesh at resolution 24: zero shell, closed, positive volume, unit normals, colours and weight_src in [0,1].
* Every C guard with sentinels; every part output optional on its own, through both entries of the one kernel; the Python guards; eval_nerf_regtr.py --merged_mesh_field on a one-scene split on disk."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import mc_restatement as M
import pair_field_restatement as PF
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import mesh, ngp
from dreg_nerf_amd import pair_field as P
from dreg_nerf_amd import render as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]


def _field(seed):
    """The generated block of tests/test_hip_render.py: random hash grid and MLPs."""
    g = torch.Generator().manual_seed(seed)
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params[:3072] = torch.randn(3072, generator=g) * 1.0
        f.mlp_base.params[3072:] = torch.randn(f.mlp_base.params.numel() - 3072, generator=g)
        f.color_mlp.params.copy_(torch.randn(7168, generator=g) * 0.2)
    return f


def _shell(res, shell):
    c = (torch.arange(res, dtype=torch.float32) + 0.5) / res * 3 - 1.5
    X, Y, Z = torch.meshgrid(c, c, c, indexing="ij")
    rad = torch.stack([X, Y, Z], -1).norm(dim=-1)
    return (rad > shell[0]) & (rad < shell[1])


def _block(seed=3, res=32, shell=(0.55, 1.05)):
    """The pair recipe of tests/test_hip_render_pair.py: (field on the device, occupancy grid with a thick shell)."""
    occ = ngp.OccupancyGrid(AABB, res)
    occ._binary.copy_(_shell(res, shell))
    return _field(seed).to(DEV).eval(), occ


def _pose():
    """POSE of tests/test_hip_render_pair.py: 25 degrees about z, then t = (-0.13, 0.02, 0.02); source frame -> target frame."""
    a = math.radians(25.0)
    Pm = torch.eye(4)
    Pm[:3, :3] = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Pm[:3, 3] = torch.tensor([-0.13, 0.02, 0.02])
    return Pm


POSE = _pose()
C_SRC, C_TGT = torch.tensor([0.3, -2.2, 0.6]), torch.tensor([2.1, 0.4, 0.5])
PARTS = ("sigma", "w_src", "w_tgt", "sigma_src", "sigma_tgt")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _empty():
    return ngp.OccupancyGrid(AABB, 32)


def _covered_torch(occ, x):
    """The coverage rule in torch fp32 elementwise ops: u = (x - lo) / ext, inside iff 0 <= u <= 1, cell clamp(floor(u res), 0, res - 1), binary != 0."""
    roi = torch.tensor(AABB, dtype=torch.float32, device=x.device)
    binary = occ.binary.to(x.device)
    u = (x - roi[:3]) / (roi[3:] - roi[:3])
    inside = ((u >= 0) & (u <= 1)).all(dim=1)
    res = torch.tensor([float(v) for v in binary.shape], dtype=torch.float32, device=x.device)
    ci = torch.minimum(torch.clamp(torch.floor(torch.where(inside[:, None], u, torch.zeros_like(u)) * res), min=0), res - 1).long()
    return inside & binary[ci[:, 0], ci[:, 1], ci[:, 2]]


def _to_source_torch(x, pose):
    """x_S in torch fp32 elementwise ops, the kernel's order: d = x - tf, x_S[k] = (Rf[0][k] d[0] + Rf[1][k] d[1]) + Rf[2][k] d[2]."""
    Rf, tf = PF.pose_f32(pose.double().numpy())
    d = [x[:, k] - float(tf[k]) for k in range(3)]
    return torch.stack([(float(Rf[0, k]) * d[0] + float(Rf[1, k]) * d[1]) + float(Rf[2, k]) * d[2] for k in range(3)], dim=1).contiguous()


def _nodes(origin, spacing, dims):
    """The lattice's node positions in torch fp32, origin_c + (float)i_c * spacing_c: [nz*ny*nx, 3], x fastest."""
    ax = [torch.tensor(origin[c], dtype=torch.float32, device=DEV) + torch.arange(dims[c], dtype=torch.float32, device=DEV) * torch.tensor(spacing[c], dtype=torch.float32, device=DEV)
          for c in range(3)]
    Z, Y, X = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return torch.stack([X, Y, Z], dim=-1).reshape(-1, 3).contiguous()


@pytest.fixture(scope="module")
def pair():
    return _block(3, shell=(0.55, 1.05)), _block(5, shell=(0.45, 0.95))


@pytest.fixture(scope="module")
def pf(pair):
    (sf, so), (tf, to) = pair
    return P.PairField(sf, so, tf, to, POSE, C_SRC, C_TGT)


@pytest.fixture(scope="module")
def ref(pair, pf):
    """The 8,192 test points, their classes from the torch statement of the coverage rule, the blocks' own queries and the kernel's parts — computed
    once and left unchanged.  Every class holds >= 400 points: no case below can be passed by absence."""
    (sf, so), (tf, to) = pair
    draw = (torch.rand(40000, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1) * 1.2
    x = draw[draw.norm(dim=1) < 1.2][:8192].contiguous().to(DEV)
    assert x.shape == (8192, 3)
    xs = _to_source_torch(x, POSE)
    m_s, m_t = _covered_torch(so, xs), _covered_torch(to, x)
    classes = {"both": m_s & m_t, "src": m_s & ~m_t, "tgt": ~m_s & m_t, "none": ~m_s & ~m_t}
    counts = {k: int(v.sum()) for k, v in classes.items()}
    print(f"classes: {counts}")
    assert min(counts.values()) >= 400, counts
    out = dict(zip(PARTS, pf.query(x, parts=True)))
    return dict(x=x, xs=xs, m_s=m_s, m_t=m_t, classes=classes, counts=counts, d_s=sf.query_raw(xs)[0], d_t=tf.query_raw(x)[0], **out)


# ------------------------------------------------------------------------------------------------------- parts and blend
def test_classes_are_the_ones_the_cases_were_chosen_on(ref):
    assert ref["counts"] == {"both": 3146, "src": 1566, "tgt": 415, "none": 3065}


def test_parts_are_the_blocks_own_queries_bit_for_bit(ref):
    assert _same(ref["sigma_tgt"], ref["d_t"] * ref["m_t"]) and _same(ref["sigma_src"], ref["d_s"] * ref["m_s"])
    assert float(ref["sigma_src"][ref["m_s"]].min()) > 0 and float(ref["sigma_tgt"][ref["m_t"]].min()) > 0
    c = ref["classes"]
    assert (ref["w_src"][c["src"]] == 1).all() and (ref["w_tgt"][c["src"]] == 0).all()
    assert (ref["w_src"][c["tgt"]] == 0).all() and (ref["w_tgt"][c["tgt"]] == 1).all()
    assert (ref["w_src"][c["none"]] == 0).all() and (ref["w_tgt"][c["none"]] == 0).all() and (ref["sigma"][c["none"]] == 0).all()
    ws, wt = ref["w_src"][c["both"]], ref["w_tgt"][c["both"]]
    assert ((ws > 0) & (ws < 1) & (wt > 0) & (wt < 1)).all()
    assert _same(wt, 1.0 - ws)                                              # w_tgt is fl(1 - w_src): the sum is 1 to that one rounding
    assert float((ws.double() + wt.double() - 1.0).abs().max()) <= 2.0 ** -24
    assert _same(ref["sigma"][c["src"]], ref["d_s"][c["src"]]) and _same(ref["sigma"][c["tgt"]], ref["d_t"][c["tgt"]])


def test_the_blend_is_exact_given_its_parts(ref):
    want = (ref["w_src"] * ref["sigma_src"]) + (ref["w_tgt"] * ref["sigma_tgt"])
    assert _same(ref["sigma"], want)
    both = ref["classes"]["both"]
    assert not _same(ref["sigma"][both], ref["sigma_src"][both]) and not _same(ref["sigma"][both], ref["sigma_tgt"][both])


def test_weight_against_fp64(ref):
    both = ref["classes"]["both"].cpu().numpy()
    xs, xt = ref["xs"].cpu().numpy()[both], ref["x"].cpu().numpy()[both]
    y = PF.log_ratio(xs, xt, C_SRC.numpy(), C_TGT.numpy(), 4.0)
    assert np.abs(y).max() <= 2.3, np.abs(y).max()                          # the premise of the bound's derivation
    want = PF.weight(xs, xt, C_SRC.numpy(), C_TGT.numpy(), 4.0)
    got = ref["w_src"].cpu().numpy()[both].astype(np.float64)
    err = float(np.abs(got - want).max())
    print(f"pair field weight: {both.sum()} shared points, max |y| {np.abs(y).max():.4f}, max |dw| {err:.3e} (derived 6.3e-7, bound 5e-6)")
    assert err <= 5e-6
    assert want.min() < 0.2 and want.max() > 0.8                             # the weight is exercised over its range, not near one value


# ------------------------------------------------------------------------------------------------------- same block twice
def test_same_block_twice_under_the_identity_is_the_masked_block(pair, ref):
    tf, to = pair[1]
    same = P.PairField(tf, to, tf, to, torch.eye(4), C_TGT, C_TGT)
    x = ref["x"]
    sigma, ws, wt, ss, st = same.query(x, parts=True)
    m = ref["m_t"]
    assert (ws[m] == 0.5).all() and (wt[m] == 0.5).all() and (ws[~m] == 0).all() and (wt[~m] == 0).all()
    assert _same(sigma, ref["d_t"] * m) and _same(ss, st) and _same(ss, ref["d_t"] * m)
    origin, spacing, dims = same.lattice(16)
    assert dims == (19, 19, 19)
    nodes = _nodes(origin, spacing, dims)
    values = (tf.query_raw(nodes)[0] * _covered_torch(to, nodes)).view(dims[2], dims[1], dims[0])
    v, f = mesh.marching_cubes(values, 0.7, origin, spacing)
    pm = P.pair_mesh(same, 16, level=0.7, normals=False, colors=False)
    assert v.shape[0] > 100 and _same(pm["verts"], v) and torch.equal(pm["faces"], f)
    assert pm["normals"] is None and pm["colors"] is None and pm["dims"] == dims


# ------------------------------------------------------------------------------------------------------- one block empty
@pytest.mark.parametrize("side", ["source_empty", "target_empty"])
def test_one_block_empty_is_the_other_block(pair, side):
    (sf, so), (tf, to) = pair
    if side == "source_empty":
        one = P.PairField(sf, _empty(), tf, to, POSE, C_SRC, C_TGT)
        field, occ, frame = tf, to, (lambda x: x)
    else:
        one = P.PairField(sf, so, tf, _empty(), POSE, C_SRC, C_TGT)
        field, occ, frame = sf, so, (lambda x: _to_source_torch(x, POSE))
    origin, spacing, dims = one.lattice(16)
    assert dims == (19, 19, 16)
    xb = frame(_nodes(origin, spacing, dims))
    values = (field.query_raw(xb)[0] * _covered_torch(occ, xb)).view(dims[2], dims[1], dims[0])
    assert _same(one.sample_lattice(origin, spacing, dims), values)
    v, f = mesh.marching_cubes(values, 0.7, origin, spacing)
    pm = P.pair_mesh(one, 16, level=0.7)
    assert v.shape[0] > 100 and _same(pm["verts"], v) and torch.equal(pm["faces"], f)
    # A vertex lies ON a lattice edge, between a node the block covers and one it may not: where the vertex's own cell is not set, the rule gives
    # the block weight 0 there, so the attributes are zeros (§3i: "zeros where the denominator is 0").  Everywhere else they are the block's own.
    vb = frame(v)
    cov = _covered_torch(occ, vb)
    assert float(cov.float().mean()) > 0.5 and int((~cov).sum()) > 0
    dirs = ngp.SampleGrid._generate_fixed_viewing_directions().to(DEV).float().contiguous()
    assert _same(pm["colors"][cov], field.query_rgb_mean(field.query_raw(vb)[1], dirs)[cov]) and not pm["colors"][~cov].any()
    own = ngp.field_normals(field, vb)
    assert float((own[cov].norm(dim=1) > 0.99).float().mean()) > 0.9 and not pm["normals"][~cov].any() and not pm["weight_src"][~cov].any()
    if side == "source_empty":
        assert _same(pm["normals"][cov], own[cov]) and (pm["weight_src"] == 0).all()
    else:
        # the source's normals arrive rotated: -R g / |R g| against R (-g / |g|).  Both are unit vectors from <= 12 fp32 operations on numbers <= 1
        # in size (|R g| and |g| agree to ~4 ulp): 16 * 2^-24 per component.  That count holds where |g|^2 is a normal fp32 number: a gradient below
        # 1e-15 in size (a point where nearly every hidden unit is off) has squares near or below 2^-126, and neither norm is accurate there.
        gsz = field.query_density_grad(vb)[1].norm(dim=1)
        sized = cov & (gsz > 1e-15)
        print(f"target empty: {int(cov.sum())} covered vertices, {int((cov & ~sized).sum())} with |grad| <= 1e-15 (smallest non-zero {float(gsz[gsz > 0].min()):.3e})")
        assert float(sized.float().sum()) >= 0.9 * float(cov.float().sum())      # (214 of 222 on this pair: the comparison is not passed by absence)
        Rm = torch.from_numpy(one.R).to(DEV)
        moved = torch.stack([Rm[k, 0] * own[:, 0] + Rm[k, 1] * own[:, 1] + Rm[k, 2] * own[:, 2] for k in range(3)], dim=1)
        assert float((pm["normals"][sized] - moved[sized]).abs().max()) <= 16 * 2.0 ** -24
        assert (pm["weight_src"][cov] == 1).all()


# ------------------------------------------------------------------------------------------------------- lattice form, order, repeatability
@pytest.mark.parametrize("lattice", ["resolution_16", "resolution_24", "nx_65"])
def test_lattice_form_is_the_points_form_of_its_nodes(pf, lattice):
    if lattice == "nx_65":
        origin, spacing, dims = [-1.3, -0.4, -0.3], [float(np.float32(0.04)), float(np.float32(0.11)), float(np.float32(0.13))], (65, 7, 5)      # the x walk straddles a wave
    else:
        origin, spacing, dims = pf.lattice(int(lattice.split("_")[1]))
        assert dims == {"resolution_16": (19, 19, 16), "resolution_24": (27, 27, 22)}[lattice]
        origin = [float(np.float32(v)) for v in origin]
    origin = [float(np.float32(v)) for v in origin]
    got = pf.sample_lattice(origin, spacing, dims)
    want = pf.query(_nodes(origin, spacing, dims))
    assert got.shape == (dims[2], dims[1], dims[0]) and _same(got.reshape(-1), want)
    assert int((got > 0.7).sum()) > 50 and int((got == 0).sum()) > 50


def test_a_permutation_permutes_and_two_runs_agree(pf, ref):
    x = ref["x"]
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    again = pf.query(x, parts=True)
    moved = pf.query(x[perm].contiguous(), parts=True)
    for k, name in enumerate(PARTS):
        assert _same(again[k], ref[name]), name
        assert _same(moved[k], ref[name][perm]), name
    assert _same(pf.query(x[:100].reshape(10, 10, 3)), ref["sigma"][:100].reshape(10, 10))
    origin, spacing, dims = pf.lattice(16)
    assert _same(pf.sample_lattice(origin, spacing, dims), pf.sample_lattice(origin, spacing, dims))


# ------------------------------------------------------------------------------------------------------- the mesh of the pair
def test_pair_mesh_is_one_closed_surface(pf):
    origin, spacing, dims = pf.lattice(24)
    assert dims == (27, 27, 22)
    values = pf.sample_lattice(origin, spacing, dims)
    shell = torch.ones_like(values, dtype=torch.bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert (values[shell] == 0).all() and int((values[~shell] > 0.7).sum()) > 100
    m = P.pair_mesh(pf, 24, level=0.7)
    verts, faces = m["verts"].cpu().numpy(), m["faces"].cpu().numpy()
    assert m["level"] == 0.7 and m["dims"] == dims and len(verts) > 500 and len(faces) > 500
    v, f = mesh.marching_cubes(values, 0.7, origin, spacing)
    assert _same(m["verts"], v) and torch.equal(m["faces"], f)
    assert M.is_closed(faces) and M.repeated_index_faces(faces) == 0 and not M.unmatched_edges(faces)
    assert M.signed_volume(verts, faces) > 0
    area, vol = mesh.mesh_area_volume(m["verts"], m["faces"])
    assert vol == pytest.approx(M.signed_volume(verts, faces), rel=1e-9) and area > 0
    n2 = (m["normals"].double() ** 2).sum(dim=1)
    assert (((n2 - 1).abs() <= 1e-5) | (n2 == 0)).all() and int((n2 > 0).sum()) > len(verts) // 2
    col, ws = m["colors"], m["weight_src"]
    assert col.shape == m["verts"].shape and float(col.min()) >= 0 and float(col.max()) <= 1
    assert ws.shape == (len(verts),) and float(ws.min()) >= 0 and float(ws.max()) <= 1 and int(((ws > 0) & (ws < 1)).sum()) > 50
    assert int((ws == 0).sum()) > 0 and int((ws == 1).sum()) > 0            # and vertices that one block alone carries
    print(f"pair_mesh resolution 24: V {len(verts)} F {len(faces)} area {area:.3f} volume {vol:.3f}; shared vertices {int(((ws > 0) & (ws < 1)).sum())}")
    bare = P.pair_mesh(pf, 24, level=0.7, normals=False, colors=False)
    assert bare["normals"] is None and bare["colors"] is None and torch.equal(bare["faces"], m["faces"]) and _same(bare["weight_src"], ws)
    assert P.pair_mesh(pf, 24)["level"] == mesh.DENSITY_THRE


# ------------------------------------------------------------------------------------------------------- guards
def test_every_c_guard_returns_einval_without_a_launch(pf, ref):
    lib = L.load()
    keep = []
    blocks = [pf._block_args(0, keep), pf._block_args(1, keep)]          # binary, rx, ry, rz, table, w1, w2, offset, size, res, scale, hashed, roi, model, center
    SENT = -77.0
    n = 256
    x = ref["x"][:n].contiguous()
    outs = [torch.full((n,), SENT, device=DEV) for _ in range(5)]
    org, spc = (ctypes.c_float * 3)(-1.0, -1.0, -1.0), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    s = L.stream()

    def call(x_=L.ptr(x), n_=n, o=None, sp=None, dims=(0, 0, 0), src=None, tgt=None, pose=pf._pose12, power=4.0, sigma=L.ptr(outs[0]), rest=None):
        rest = [L.ptr(t) for t in outs[1:]] if rest is None else rest
        return lib.dreg_pair_density(x_, n_, o, sp, *dims, *(blocks[0] if src is None else src), *(blocks[1] if tgt is None else tgt), pose, power, sigma, *rest, s)

    def without(k, i, v=None):
        b = list(blocks[k])
        b[i] = v
        return b
    bad = [call(x_=None), call(sigma=None), call(pose=None), call(n_=-1), call(n_=-1, x_=None)]
    for k, key in ((0, "src"), (1, "tgt")):
        bad += [call(**{key: without(k, i)}) for i in (0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)]       # every pointer of the block
        bad += [call(**{key: without(k, i, v)}) for i, v in ((1, 0), (2, -1), (3, 0))]                     # an occupancy-grid dimension <= 0
    bad += [call(power=p) for p in (0.0, -1.0, float("nan"), float("inf"), -float("inf"))]
    lat = lambda **kw: call(**{**dict(x_=None, n_=0, o=org, sp=spc, dims=(4, 4, 4)), **kw})
    bad += [lat(dims=d) for d in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -3, 4), (1025, 4, 4), (4, 1025, 4), (4, 4, 1025), (1024, 1024, 257))]
    bad += [lat(o=None), lat(sp=None), lat(x_=L.ptr(x)), lat(sigma=None), lat(pose=None), lat(n_=-1), lat(power=0.0), lat(src=without(0, 0)), lat(tgt=without(1, 3, 0))]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs), "a refused call wrote to the device"
    # n == 0: OK, nothing launched, whatever the pointers
    assert call(n_=0) == 0 and call(n_=0, x_=None, sigma=None, rest=[None] * 4) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs)
    assert pf.query(torch.empty(0, 3, device=DEV)).shape == (0,)
    # the optional outputs are optional; a good call writes what the wrapper returns
    assert call(rest=[None] * 4) == 0
    torch.cuda.synchronize()
    assert _same(outs[0], ref["sigma"][:n]) and all(bool((t == SENT).all()) for t in outs[1:])
    assert call() == 0
    torch.cuda.synchronize()
    for k, name in enumerate(PARTS):
        assert _same(outs[k], ref[name][:n]), name
    small = torch.full((64,), SENT, device=DEV)
    assert lat(sigma=L.ptr(small), rest=[None] * 4) == 0
    torch.cuda.synchronize()
    assert _same(small.view(4, 4, 4), pf.sample_lattice([-1.0] * 3, [0.25] * 3, (4, 4, 4)))


def test_every_part_output_is_optional_on_its_own(pair, pf, ref):
    """The per-block part outputs go out through one nullable pointer per block and array.  n = 65 points (one full chunk plus one lane, points of
    all four coverage classes): with any one part pointer of dreg_pair_density given and the other three null, and with w_tgt + sigma_src alone,
    the arrays asked for hold the bytes of the all-parts call, the others are untouched and sigma is the same every time; the same for
    dreg_scene_density at K = 3 with weight_block alone and with sigma_block alone."""
    from dreg_nerf_amd import scene_field as S
    lib = L.load()
    keep = []
    blocks = [pf._block_args(0, keep), pf._block_args(1, keep)]
    n, SENT, s = 65, -77.0, L.stream()
    x = torch.cat([ref["x"][ref["classes"][k]][:17] for k in ("both", "src", "tgt", "none")])[:n].contiguous()
    assert x.shape == (n, 3)

    def pair_call(asked):
        outs = [torch.full((n,), SENT, device=DEV) for _ in range(5)]
        rest = [L.ptr(outs[k]) if k in asked else None for k in range(1, 5)]
        assert lib.dreg_pair_density(L.ptr(x), n, None, None, 0, 0, 0, *blocks[0], *blocks[1], pf._pose12, pf.power, L.ptr(outs[0]), *rest, s) == 0
        torch.cuda.synchronize()
        return outs

    full = pair_call({1, 2, 3, 4})
    for got, want in zip(full, pf.query(x, parts=True)):
        assert _same(got, want)
    assert bool(((full[1] > 0) & (full[1] < 1)).any()) and bool((full[1] == 1).any()) and bool((full[2] == 1).any()) and bool((full[0] == 0).any())
    for asked in ({1}, {2}, {3}, {4}, {2, 3}):
        got = pair_call(asked)
        assert _same(got[0], full[0]), asked
        for k in range(1, 5):
            assert _same(got[k], full[k]) if k in asked else bool((got[k] == SENT).all()), (asked, PARTS[k])

    (sf, so), (tf, to) = pair
    third = torch.eye(4)
    third[:3, 3] = torch.tensor([0.2, -0.1, 0.15])
    sc = S.SceneField([(sf, so, C_SRC, POSE), (tf, to, C_TGT, None), (sf, so, C_SRC, third)])
    arr = sc._block_array(keep)

    def scene_call(want_w, want_s):
        sigma, wb, sb = torch.full((n,), SENT, device=DEV), torch.full((n, 3), SENT, device=DEV), torch.full((n, 3), SENT, device=DEV)
        assert lib.dreg_scene_density(L.ptr(x), n, None, None, 0, 0, 0, 3, ctypes.cast(arr, ctypes.c_void_p), sc.power, L.ptr(sigma),
                                      L.ptr(wb) if want_w else None, L.ptr(sb) if want_s else None, s) == 0
        torch.cuda.synchronize()
        return sigma, wb, sb

    full3 = scene_call(True, True)
    for got, want in zip(full3, sc.query(x, parts=True)):
        assert _same(got, want)
    assert bool(((full3[1] > 0).sum(dim=1) == 3).any())                     # some point is shared by all three blocks
    only_w, only_s = scene_call(True, False), scene_call(False, True)
    assert _same(only_w[0], full3[0]) and _same(only_w[1], full3[1]) and bool((only_w[2] == SENT).all())
    assert _same(only_s[0], full3[0]) and _same(only_s[2], full3[2]) and bool((only_s[1] == SENT).all())


def test_python_guards(pair, pf):
    (sf, so), (tf, to) = pair
    sf.unbounded = True
    try:
        with pytest.raises(NotImplementedError):
            P.PairField(sf, so, tf, to, POSE, C_SRC, C_TGT)
        with pytest.raises(NotImplementedError):
            P.PairField(tf, to, sf, so, POSE, C_SRC, C_TGT)
    finally:
        sf.unbounded = False
    contracted = R.BlockGrid(AABB, so.binary.to(DEV).view(torch.uint8), contraction_type=ngp.ContractionType.UN_BOUNDED_SPHERE)
    with pytest.raises(NotImplementedError):
        P.PairField(sf, contracted, tf, to, POSE, C_SRC, C_TGT)
    with pytest.raises(NotImplementedError):
        P.PairField(sf, so, tf, contracted, POSE, C_SRC, C_TGT)
    cpu_field = ngp.NGPradianceField(AABB).eval()
    with pytest.raises(ValueError):
        P.PairField(cpu_field, so, tf, to, POSE, C_SRC, C_TGT)
    with pytest.raises(ValueError):
        P.PairField(sf, so, cpu_field, to, POSE, C_SRC, C_TGT)
    for power in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.PairField(sf, so, tf, to, POSE, C_SRC, C_TGT, power=power)
    with pytest.raises(ValueError):
        P.PairField(sf, so, tf, to, torch.eye(3), C_SRC, C_TGT)
    with pytest.raises(ValueError):
        pf.query(torch.zeros(4, 3))
    for dims in ((1, 4, 4), (4, 4, 1025), (1024, 1024, 257)):
        with pytest.raises(ValueError):
            pf.sample_lattice([0.0] * 3, [0.1] * 3, dims)
    blk = R.BlockGrid(AABB, so.binary.to(DEV).view(torch.uint8))
    assert _same(P.PairField(sf, blk, tf, to, POSE[:3], C_SRC, C_TGT).query(torch.zeros(1, 3, device=DEV) + 0.7), pf.query(torch.zeros(1, 3, device=DEV) + 0.7))


# ------------------------------------------------------------------------------------------------------- the evaluator's flag on disk
def _write_block(path, seed, res=64):
    """_write_block of tests/test_hip_marching_cubes.py: a generated block's checkpoint with six cameras."""
    occ = ngp.OccupancyGrid(AABB, res)
    occ._binary.copy_(_shell(res, (0.55, 1.05)))
    cams = torch.eye(4)[None].repeat(6, 1, 1)
    cams[:, :3, 3] = torch.tensor([[2.5, 0, 0], [-2.5, 0, 0], [0, 2.5, 0], [0, -2.5, 0], [0, 0, 2.5], [0, 0, -2.5]]) + torch.tensor([0.3 * seed - 1.5, 0.2, 0.1])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"step": 1, "model": _field(seed).state_dict(), "occupancy_grid": occ.state_dict(), "aabb": AABB, "unbounded": False, "near_plane": None, "far_plane": None,
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


def _without_time(path):
    """metrics_test.json with the wall-clock entry of every scene row set to 0, serialised as the evaluator serialises it.  `time` is a host clock
    around the forward call and differs between ANY two runs; every other byte of the file is held equal."""
    m = json.load(open(path))
    for row in m.values():
        if isinstance(row, dict) and "time" in row:
            row["time"] = 0.0
    return json.dumps(m, indent=2).encode()


def test_merged_mesh_field_writes_one_closed_surface_per_pose(tmp_path, monkeypatch, capsys):
    """eval_nerf_regtr.py --merged_mesh_field (its main(), in this process) on the one-scene split of tests/test_hip_marching_cubes.py."""
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
    reg = common + ["--json_dir", jd]
    _main(monkeypatch, "eval_nerf_regtr", reg + ["--expname", "plain"])
    _main(monkeypatch, "eval_nerf_regtr", reg + ["--expname", "field", "--merged_mesh_field"])
    out = capsys.readouterr().out
    assert "merged field mesh" in out and "merged_field_mesh_{pred,gt}.ply" in out
    base = lambda name: os.path.join(root, "eval", name, "objaverse")
    assert _without_time(os.path.join(base("field"), "metrics_test.json")) == _without_time(os.path.join(base("plain"), "metrics_test.json"))
    d = os.path.join(base("field"), "sceneA")
    assert sorted(os.listdir(d)) == ["merged_field_mesh.json", "merged_field_mesh_gt.ply", "merged_field_mesh_pred.ply"]
    assert not os.path.exists(os.path.join(base("plain"), "sceneA"))
    stats = json.load(open(os.path.join(d, "merged_field_mesh.json")))
    for name in ("pred", "gt"):
        v, f, c, nrm = vis_dump.read_mesh_ply(os.path.join(d, f"merged_field_mesh_{name}.ply"))
        st = stats[name]
        assert set(st) == {"V", "F", "area", "volume"} and st["V"] == len(v) > 100 and st["F"] == len(f) > 100
        assert c.shape == v.shape and nrm.shape == v.shape and M.is_closed(f) and M.repeated_index_faces(f) == 0
        area, vol = mesh.mesh_area_volume(torch.from_numpy(v), torch.from_numpy(f))
        assert st["area"] == pytest.approx(area, rel=1e-12) and st["volume"] == pytest.approx(vol, rel=1e-12) and vol > 0 and area > 0
    assert stats["level"] == 0.7 and stats["resolution"] == res
    # the gt file is the pair's mesh under the known pose: which block was the source is the dataset's draw (quirk Q15), so one of the two orders gives it
    gt = vis_dump.read_mesh_ply(os.path.join(d, "merged_field_mesh_gt.ply"))
    matched = False
    for s_, t_ in ((0, 1), (1, 0)):
        blocks = [R.load_render_block(ck[k], DEV) for k in (s_, t_)]
        cen = [torch.as_tensor(b[2]["camera_poses"]).float()[:, :3, 3].mean(0) for b in blocks]
        pose = transforms[t_] @ torch.linalg.inv(transforms[s_])
        m = P.pair_mesh(P.PairField(blocks[0][0], blocks[0][1], blocks[1][0], blocks[1][1], pose, cen[0], cen[1]), res)
        if len(gt[0]) == m["verts"].shape[0] and np.array_equal(gt[0], m["verts"].cpu().numpy().astype(np.float64)) and np.array_equal(gt[1], m["faces"].cpu().numpy()):
            matched = True
    assert matched, "merged_field_mesh_gt.ply is not the pair's mesh under the known pose in either block order"
