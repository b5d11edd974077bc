"""CPU: the host side of the K-block renderer and of whole-scene registration.  The CPU restatement of the K-block rule
(tests/render_scene_restatement.py) against closed forms on test_render_pair_host.py's constant-field slabs and against the pair's restatement;
the flags; the files and schemas of eval_nerf_regtr.py --register_scene / --render_scene with an injected pair_fn / renderer; get_scene."""
import importlib
import json
import math
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import render_pair_restatement as RP
import render_scene_restatement as RS
from dreg_nerf_amd import dataset as D
from dreg_nerf_amd import render as R
from dreg_nerf_amd import scene_reg, synth
from dreg_nerf_amd.config import config_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AABB = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
RED, GREEN, BLUE = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)


def _slab(z_cells):
    b = torch.zeros(8, 8, 8, dtype=torch.bool)                      # cells of 0.25 over [-1, 1]
    b[:, :, z_cells] = True
    return b


def _const_field(sigma, rgb):
    return lambda x, d: (torch.full((x.shape[0],), float(sigma)), torch.tensor(rgb).expand(x.shape[0], 3))


def _block(field, binary, dt, center=(0.0, 0.0, -3.0), **kw):
    return dict(field=field, binary=binary, roi_aabb=AABB, scene_aabb=AABB, dt=dt, center=center, **kw)


def _z_rays():
    o = torch.tensor([[-0.3, 0.1, -3.0], [0.2, -0.5, -3.0], [0.0, 0.0, -3.0]])
    d = torch.tensor([[0.0, 0.0, 1.0]]).expand(3, 3).contiguous()
    return o, d


# ------------------------------------------------------------------------------------------------------- the restatement vs closed forms
def test_three_disjoint_slabs_front_over_middle_over_back():
    """Slabs z in [-1, -0.5), [-0.25, 0.25), [0.5, 1), each on its own step, listed back, front, middle: the order is the depth's, not the list's."""
    sig, L = (1.5, 0.8, 1.1), 0.5
    front = _block(_const_field(sig[0], RED), _slab(slice(0, 2)), 0.1)
    middle = _block(_const_field(sig[1], GREEN), _slab(slice(3, 5)), 0.05)
    back = _block(_const_field(sig[2], BLUE), _slab(slice(6, 8)), 0.125)
    rays = _z_rays()
    out = RS.render_scene([back, front, middle], [rays] * 3, bkgd=(1.0, 1.0, 1.0))
    e = [math.exp(-s * L) for s in sig]
    tol = max(sig[0] * 0.1, sig[1] * 0.05, sig[2] * 0.125)          # the lattice error of a slab's optical depth
    assert (out["omega"] == 1).all() and (out["n_cover"] == 0).all()
    assert (out["opacity"] - (1 - e[0] * e[1] * e[2])).abs().max().item() <= tol
    want = torch.tensor(RED) * (1 - e[0]) + e[0] * (1 - e[1]) * torch.tensor(GREEN) + e[0] * e[1] * (1 - e[2]) * torch.tensor(BLUE) + e[0] * e[1] * e[2] * torch.ones(3)
    assert (out["rgb"] - want).abs().max().item() <= tol
    wb = torch.tensor([e[0] * e[1] * (1 - e[2]), 1 - e[0], e[0] * (1 - e[1])])       # in the list's order: back, front, middle
    assert (out["weight_block"] - wb).abs().max().item() <= tol
    assert out["n_samples"] == 3 * (5 + 10 + 4)
    first = out["block"][:, 0]
    assert (first == 1).all() and (out["block"][:, 5] == 2).all() and (out["block"][:, 15] == 0).all()


def test_three_coincident_slabs_are_counted_once():
    """Three blocks model the same slab z in [-0.5, 0.5) and their cameras share a centroid: omega = 1/3 each, the scene renders the single
    slab — told apart from 1 - exp(-3 sigma L), what triple counting gives."""
    sigma, L, dt = 1.0, 1.0, 0.05
    mk = lambda: _block(_const_field(sigma, RED), _slab(slice(2, 6)), dt)
    rays = _z_rays()
    out = RS.render_scene([mk(), mk(), mk()], [rays] * 3)
    marched = out["alpha"] > 0
    assert marched.any() and (out["n_cover"][marched] == 2).all()
    assert (out["omega"][marched] - 1.0 / 3.0).abs().max().item() <= 1e-7
    single, triple = 1 - math.exp(-sigma * L), 1 - math.exp(-3 * sigma * L)
    tol = sigma * dt
    assert (out["opacity"] - single).abs().max().item() <= tol
    assert (out["weight_block"] - single / 3).abs().max().item() <= tol
    naive = RS.render_scene([mk(), mk(), mk()], [rays] * 3, use_omega=False)
    assert (naive["opacity"] - triple).abs().max().item() <= tol and triple - single > 2 * tol
    # unequal centroids: the covering blocks' weights still sum to 1 at a shared parameter, and the nearest camera takes the most
    near = lambda c: _block(_const_field(sigma, RED), _slab(slice(2, 6)), dt, center=c)
    o3 = RS.render_scene([near((0.0, 0.0, -1.0)), near((0.0, 0.0, -2.0)), near((0.0, 0.0, -3.0))], [(rays[0][2:], rays[1][2:])] * 3, power=2.0)
    k = int(torch.nonzero(o3["alpha"][0] > 0)[0])
    om = o3["omega"][0, k:k + 3]
    assert torch.equal(o3["block"][0, k:k + 3], torch.tensor([0, 1, 2])) and torch.equal(o3["t"][0, k:k + 3], o3["t"][0, k].expand(3))
    assert abs(float(om.sum()) - 1.0) <= 1e-6 and om[0] > om[1] > om[2]
    z = -3.0 + float(o3["t"][0, k])
    inv = [1 / (z + 1.0) ** 2, 1 / (z + 2.0) ** 2, 1 / (z + 3.0) ** 2]           # p = 2: omega_b proportional to 1 / delta_b
    assert (om - torch.tensor(inv) / sum(inv)).abs().max().item() <= 1e-6


def test_two_coincident_slabs_plus_one_disjoint():
    """Blocks 0 and 2 share the slab z in [-0.5, 0), block 1 holds z in [0.5, 1) alone: the shared slab counts once (the pair's omega = 1/2), the
    far slab fully behind it."""
    sigma, dt = 1.2, 0.05
    shared = lambda: _block(_const_field(sigma, RED), _slab(slice(2, 4)), dt)
    far = _block(_const_field(0.9, GREEN), _slab(slice(6, 8)), dt)
    rays = _z_rays()
    out = RS.render_scene([shared(), far, shared()], [rays] * 3)
    m = out["alpha"] > 0
    assert (out["omega"][m & (out["block"] != 1)] == 0.5).all() and (out["omega"][m & (out["block"] == 1)] == 1).all()
    assert (out["n_cover"][m & (out["block"] != 1)] == 1).all() and (out["n_cover"][m & (out["block"] == 1)] == 0).all()
    e_s, e_f = math.exp(-sigma * 0.5), math.exp(-0.9 * 0.5)
    tol = sigma * dt
    assert (out["opacity"] - (1 - e_s * e_f)).abs().max().item() <= tol
    assert (out["weight_block"] - torch.tensor([0.5 * (1 - e_s), e_s * (1 - e_f), 0.5 * (1 - e_s)])).abs().max().item() <= tol


def test_tie_order_lowest_index_first():
    """Equal lattices and three opaque blocks: every t_mid is a three-way tie, composited in the list's order."""
    dt = 0.1
    rays = _z_rays()
    mk = lambda c: _block(_const_field(1e3, c), _slab(slice(2, 6)), dt)
    out = RS.render_scene([mk(RED), mk(GREEN), mk(BLUE)], [rays] * 3)
    assert torch.equal(out["t"][:, 0], out["t"][:, 1]) and torch.equal(out["t"][:, 1], out["t"][:, 2])
    assert torch.equal(out["block"][:, :6], torch.tensor([0, 1, 2, 0, 1, 2]).expand(3, 6))
    # the first sample of every block carries omega = 1/3, so the first block takes 1 - exp(-1e3 * 0.1 / 3) ~ 1 of the ray
    assert (out["rgb"] - torch.tensor(RED)).abs().max().item() <= 1e-6 and (out["weight_block"][:, 0] - out["opacity"]).abs().max().item() <= 1e-6
    swapped = RS.render_scene([mk(BLUE), mk(GREEN), mk(RED)], [rays] * 3)
    assert (swapped["rgb"] - torch.tensor(BLUE)).abs().max().item() <= 1e-6


def test_weight_block_sums_to_the_opacity():
    rays = _z_rays()
    blocks = [_block(_const_field(0.7, RED), _slab(slice(1, 5)), 0.1, center=(0.0, 0.0, -1.5)), _block(_const_field(1.3, GREEN), _slab(slice(3, 7)), 0.05),
              _block(_const_field(0.4, BLUE), _slab(slice(2, 8)), 0.08, center=(0.5, 0.0, -2.0)), _block(_const_field(2.0, RED), _slab(slice(4, 6)), 0.03)]
    for n in (1, 2, 3, 4):
        out = RS.render_scene(blocks[:n], [rays] * n, bkgd=(1.0, 1.0, 1.0))
        assert out["weight_block"].shape == (3, n) and (out["weight_block"].sum(1) - out["opacity"]).abs().max().item() <= 1e-6
        assert (out["weight_block"] > 0).all()
    assert (out["n_cover"] >= 2).any() and (out["n_cover"] == 3).any()


def test_two_blocks_equal_the_pair_restatement_exactly():
    rays = _z_rays()
    g = torch.Generator().manual_seed(3)
    d = torch.nn.functional.normalize(torch.tensor([[0.1, 0.05, 1.0], [-0.2, 0.1, 1.0], [0.0, 0.3, 1.0]]), dim=-1)
    rays_b = (rays[0] + 0.05 * torch.randn(3, 3, generator=g), d)
    src = _block(_const_field(0.7, RED), _slab(slice(1, 5)), 0.1, center=(0.3, 0.0, -1.5), alpha_thre=1e-2)
    tgt = _block(_const_field(1.3, GREEN), _slab(slice(3, 7)), 0.05, center=(0.0, -0.4, -3.0), near_plane=2.1)
    for power in (4.0, 1.5):
        want = RP.render_pair(src, tgt, rays_b, rays, power=power, bkgd=(1.0, 1.0, 1.0))
        got = RS.render_scene([src, tgt], [rays_b, rays], power=power, bkgd=(1.0, 1.0, 1.0))
        assert ((want["omega"] < 1) & want["surv"]).any()
        for k in ("rgb", "opacity", "depth", "t", "omega", "alpha", "surv"):
            assert torch.equal(got[k], want[k]), k
        assert torch.equal(got["weight_block"][:, 0], want["weight_src"]) and got["n_samples"] == want["n_samples"]
        assert torch.equal(got["block"] == 0, want["is_src"])
    # and one block is the one-block rule
    import render_restatement as RR
    one = RR.render(src["field"], rays[0], rays[1], src["binary"], AABB, AABB, 0.1, bkgd=(1.0, 1.0, 1.0), alpha_thre=1e-2)
    got = RS.render_scene([src], [rays], bkgd=(1.0, 1.0, 1.0))
    assert got["n_samples"] == one[3] and (got["rgb"] - one[0]).abs().max().item() <= 1e-6 and torch.equal(got["weight_block"][:, 0], got["opacity"])


# ------------------------------------------------------------------------------------------------------- flags, synth, get_scene
def test_flags_parse():
    cfg = config_parser([])
    assert cfg.register_scene is False and cfg.scene_robust is False and cfg.render_scene is False and cfg.synthetic_blocks == 2
    cfg = config_parser(["--register_scene", "--scene_robust", "--synthetic_blocks", "4", "--render_scene"])
    assert cfg.register_scene and cfg.scene_robust and cfg.render_scene and cfg.synthetic_blocks == 4 and cfg.render_merged is False


def test_shell_scene_generalises_shell_pair_and_the_default_dataset_is_unchanged():
    pose = synth.fixed_pose()
    pair = synth.shell_pair(16, 1, 2, pose=pose)
    scene = synth.shell_scene(16, (1, 2, 5), [torch.eye(4), pose, synth.fixed_pose(1)])
    assert len(scene) == 3 and [b["block_id"] for b in scene] == [0, 1, 2]
    assert torch.equal(scene[0]["xyz_rgba"], pair["src_xyz_rgba"]) and torch.equal(scene[1]["xyz_rgba"], pair["tgt_xyz_rgba"])
    assert torch.equal(scene[0]["mask"], pair["src_mask"]) and torch.equal(scene[1]["mask"], pair["tgt_mask"])
    s01 = scene_reg.pair_sample(scene, 0, 1)
    assert torch.equal(s01["pose"], pair["pose"]) and torch.equal(s01["tgt_xyz_rgba"], pair["tgt_xyz_rgba"]) and s01["block_list"] == [0, 1]
    # the ground truth maps block i to the anchor: G_1 = inv(pose)
    G = scene_reg.ground_truth(scene)
    assert torch.equal(G[0], torch.eye(4, dtype=torch.float64)) and (G[1] - torch.linalg.inv(pose.double())).abs().max().item() <= 1e-12
    with pytest.raises(ValueError):
        synth.shell_scene(16, (1, 2), [torch.eye(4)])
    # SyntheticRegDataset: the default and n_blocks = 3 give the same samples; get_scene's first two blocks are that sample's
    a, b = D.SyntheticRegDataset(2, 16, "test"), D.SyntheticRegDataset(2, 16, "test", n_blocks=3)
    for k, v in a[1].items():
        assert torch.equal(v, b[1][k]) if torch.is_tensor(v) else v == b[1][k], k
    sc = b.get_scene(1)
    assert len(sc) == 3 and len(a.get_scene(1)) == 2 and sc[0]["scene"] == a[1]["scene"]
    assert torch.equal(sc[1]["xyz_rgba"], a[1]["tgt_xyz_rgba"]) and torch.equal(scene_reg.pair_sample(sc, 0, 1)["pose"], a[1]["pose"])
    with pytest.raises(ValueError):
        D.SyntheticRegDataset(1, 16, "test", n_blocks=5)


def test_get_scene_on_a_hand_made_three_block_tree(tmp_path):
    root, jd = tmp_path / "data", tmp_path / "json"
    T = {0: torch.eye(4), 2: synth.fixed_pose(), 5: synth.fixed_pose(1), 7: torch.eye(4)}          # block 7 has no files: not usable
    (root / "objaverse" / "images" / "sceneA").mkdir(parents=True)
    jd.mkdir()
    json.dump({str(k): v.tolist() for k, v in T.items()}, open(root / "objaverse" / "images" / "sceneA" / "world_frame_transforms.json", "w"))
    json.dump({"train": [], "test": ["sceneA"]}, open(jd / "objaverse.json", "w"))
    for k in (5, 0, 2):
        d = root / "objaverse" / "nerf_models" / "sceneA" / f"block_{k}"
        d.mkdir(parents=True)
        g, m = synth.shell_grid(8, 10 + k, 0.5, 1.2, pose=T[k])
        torch.save(g, d / "voxel_grid.pt")
        torch.save(m, d / "voxel_mask.pt")
    ds = D.NeRFRegDataset(str(root), str(jd), "objaverse", "test")
    state = (random.getstate(), torch.get_rng_state())
    scene = ds.get_scene(0)
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])          # no random stream is drawn from
    assert [b["block_id"] for b in scene] == [0, 2, 5] and all(b["scene"] == "sceneA" and b["index"] == 0 for b in scene)
    for b in scene:
        k = b["block_id"]
        assert torch.equal(b["transform"], T[k]) and b["nerf_path"].endswith(os.path.join(f"block_{k}", "model.pth"))
        g, m = synth.shell_grid(8, 10 + k, 0.5, 1.2, pose=T[k])
        assert torch.equal(b["xyz_rgba"], g.permute(3, 2, 0, 1).unsqueeze(0)) and torch.equal(b["mask"], m)
    # consistent with get: the pair (i, j) of the scene carries get's pose for that block order
    pair = ds.get(0, block_order=[2, 5, 0])
    s = scene_reg.pair_sample(scene, 1, 2)
    assert torch.equal(s["pose"], pair["pose"]) and torch.equal(s["src_xyz_rgba"], pair["src_xyz_rgba"]) and s["block_list"] == pair["block_list"]
    G = scene_reg.ground_truth(scene)
    assert (G[2] - (T[0].double() @ torch.linalg.inv(T[5].double()))).abs().max().item() <= 1e-12
    # the sparse form, which is what the evaluator reads: the same blocks as (idx, vals), moved to the dataset's device, and the pair sample of
    # such a scene is get's for that block order (a SparseBlock moves with .to, like a tensor)
    sds = D.NeRFRegDataset(str(root), str(jd), "objaverse", "test", sparse=True, device="cpu")
    sparse = sds.get_scene(0)
    assert [b["block_id"] for b in sparse] == [0, 2, 5] and all("xyz_rgba" not in b and isinstance(b["sparse"], D.SparseBlock) for b in sparse)
    for b, dense in zip(sparse, scene):
        assert torch.equal(b["sparse"].dense(), dense["xyz_rgba"]) and torch.equal(b["sparse"].idx, dense["mask"]) and torch.equal(b["transform"], dense["transform"])
    pair = sds.get(0, block_order=[5, 0, 2])
    s = scene_reg.pair_sample(sparse, 2, 0, device="cpu")
    assert set(s) == set(pair) and torch.equal(s["pose"], pair["pose"]) and s["block_list"] == pair["block_list"] and s["src_nerf_path"] == pair["src_nerf_path"]
    for side in ("src_sparse", "tgt_sparse"):
        assert isinstance(s[side], D.SparseBlock) and torch.equal(s[side].idx, pair[side].idx) and torch.equal(s[side].vals, pair[side].vals) and s[side].res == pair[side].res
    res = scene_reg.register_scene(None, sparse, pair_fn=lambda i, j, smp: smp["pose"][0], device="cpu")
    assert (res["G"] - G).abs().max().item() <= 1e-6 and len(res["edges"]) == 6


# ------------------------------------------------------------------------------------------------------- --register_scene / --render_scene
def _evaluator():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("eval_nerf_regtr")


def _gt_pair_fn(noise_deg=0.0):
    def fn(i, j, sample):
        P = sample["pose"][0].double()
        if noise_deg and (i, j) == (1, 0):                           # the direct edge block 1 -> anchor is off; the cycles through block 2 say so
            a = math.radians(noise_deg)
            Rz = torch.tensor([[math.cos(a), -math.sin(a), 0, 0], [math.sin(a), math.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64)
            P = Rz @ P
        return P[:3]                                                 # [3,4], as the model returns it
    return fn


def test_register_scene_writes_its_file_and_leaves_metrics_and_rng_alone(tmp_path):
    E = _evaluator()
    cfg = config_parser(["--register_scene", "--scene_robust", "--root_dir", str(tmp_path), "--expname", "t", "--dataset", ""])
    ds = D.SyntheticRegDataset(2, 8, "test", n_blocks=3)
    d = tmp_path / "eval" / "t" / "synthetic"
    d.mkdir(parents=True)
    metrics = d / "metrics_test.json"
    metrics.write_text(json.dumps({"shell_0000": {"R_mean": 1.0, "t_mean": 0.1, "R_med": 1.0, "t_med": 0.1, "time": 0.5}, "R_mean": 1.0, "t_mean": 0.1}, indent=2))
    before = metrics.read_bytes()
    state = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state())
    rows = E.register_scenes(cfg, ds, None, "cpu", pair_fn=_gt_pair_fn(25.0), log=lambda *a, **k: None)
    out = E.write_scenes(str(d), "test", rows, log=lambda *a, **k: None)
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1]) and torch.equal(torch.get_rng_state(), state[2])
    assert metrics.read_bytes() == before and sorted(os.listdir(d)) == ["metrics_test.json", "scene_metrics_test.json"]
    js = json.loads((d / "scene_metrics_test.json").read_text())
    assert js == out and set(js) == {"shell_0000", "shell_0001", "R_mean", "t_mean", "R_mean_direct", "t_mean_direct"}
    row = js["shell_0001"]
    assert set(row) == {"blocks", "edges", "R_mean", "t_mean", "R_mean_direct", "t_mean_direct"}
    assert [b["block"] for b in row["blocks"]] == [0, 1, 2] and all(set(b) == {"block", "rre", "rte", "rre_direct", "rte_direct"} for b in row["blocks"])
    assert [(e["i"], e["j"]) for e in row["edges"]] == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    assert all(set(e) == {"i", "j", "residual_rot_deg", "residual_trans", "weight"} for e in row["edges"])
    # the wrong direct edge: 25 degrees pairwise, the robust synchronisation gives it no weight and recovers the block
    b1 = row["blocks"][1]
    assert b1["rre_direct"] == pytest.approx(25.0, abs=1e-3) and b1["rre"] < 0.1 and row["edges"][2]["weight"] < 0.05 and row["edges"][2]["residual_rot_deg"] > 20
    assert row["blocks"][0] == {"block": 0, "rre": 0.0, "rte": 0.0, "rre_direct": 0.0, "rte_direct": 0.0}
    assert js["R_mean"] == pytest.approx(np.mean([js[s]["R_mean"] for s in ("shell_0000", "shell_0001")])) and js["R_mean_direct"] > 5 > js["R_mean"]
    # plain least squares spreads it instead
    cfg.scene_robust = False
    plain = E.register_scenes(cfg, ds, None, "cpu", pair_fn=_gt_pair_fn(25.0), log=lambda *a, **k: None)
    assert plain["shell_0001"]["blocks"][1]["rre"] > 4.0 and all(e["weight"] == 1.0 for e in plain["shell_0001"]["edges"])


def test_render_scene_files_and_metrics_schema(tmp_path, monkeypatch):
    E = _evaluator()
    W, H = 8, 6
    monkeypatch.setitem(R.INTRINSICS, "objaverse", (W, H, 7.0, 7.0, 4.0, 3.0))
    g = torch.Generator().manual_seed(0)
    T = [torch.eye(4), synth.fixed_pose(), synth.fixed_pose(1)]
    scene = synth.shell_scene(8, (1, 2, 3), T)
    cams = []
    for k, b in enumerate(scene):
        c = torch.eye(4).repeat(k + 1, 1, 1)                        # 1, 2 and 3 cameras
        c[:, :3, 3] = torch.randn(k + 1, 3, generator=g)
        cams.append(c)
        b["nerf_path"] = str(tmp_path / f"block_{k}.pth")
        torch.save({"camera_poses": c}, b["nerf_path"])
        b.update({"scene": "sceneA", "dataset": "objaverse", "index": 0})

    class DS:
        def __len__(self):
            return 1

        def get_scene(self, i):
            return scene
    seen = []

    def stub(poses, views, K, W_, H_):
        assert (W_, H_) == (W, H) and torch.equal(K, R.intrinsics("objaverse")[0])
        seen.append((torch.as_tensor(poses).clone(), views.clone()))
        n = views.shape[0]
        level = 0.25 * len(seen)
        share = torch.zeros(H, W, 3)
        share[..., 1] = 1.0
        return [torch.full((H, W, 3), level) for _ in range(n)], [torch.linspace(0, 1, H * W).reshape(H, W, 1) for _ in range(n)], [share for _ in range(n)]

    def metrics(pred, gt):
        assert len(pred) == len(gt) == 6 and float(pred[0][0, 0, 0]) == 0.5 and float(gt[0][0, 0, 0]) == 0.25      # aligned against gt
        return [20.0 + i for i in range(6)], [0.4 + 0.1 * i for i in range(6)]

    cfg = config_parser(["--register_scene", "--render_scene", "--root_dir", str(tmp_path), "--expname", "t", "--dataset", "objaverse"])
    rows = E.register_scenes(cfg, DS(), None, "cpu", pair_fn=_gt_pair_fn(), renderer=stub, metrics=metrics, log=lambda *a, **k: None)
    assert set(rows) == {"sceneA"} and rows["sceneA"]["R_mean"] < 0.1
    G_gt = scene_reg.ground_truth(scene)
    # (the edges are the samples' fp32 poses, as the network would return them: the synchronised G is the ground truth to fp32 rounding)
    assert len(seen) == 2 and torch.equal(seen[0][0], G_gt) and (seen[1][0] - G_gt).abs().max().item() <= 1e-6
    want_views = torch.cat([(G_gt[b] @ cams[b].double()).float() for b in range(3)])
    assert torch.equal(seen[0][1], want_views) and torch.equal(seen[1][1], want_views)                # every block's cameras, in the anchor frame
    out = tmp_path / "eval" / "t" / "objaverse" / "sceneA"
    for prefix in ("gt", "aligned"):
        d = out / f"{prefix}_scene_images"
        names = [f"{kind}_{i}.png" for kind in ("rgb", "depth") for i in range(6)] + [f"share_{b}_{i}.png" for b in range(3) for i in range(6)]
        assert sorted(p.name for p in d.iterdir()) == sorted(names)
        for p in d.iterdir():
            im = Image.open(p)
            assert im.size == (W, H) and im.mode == "RGB", p
        assert (np.asarray(Image.open(d / "share_1_3.png")) == 255).all() and (np.asarray(Image.open(d / "share_0_3.png")) == 0).all()
    assert (np.asarray(Image.open(out / "gt_scene_images" / "rgb_0.png")) == 63).all() and (np.asarray(Image.open(out / "aligned_scene_images" / "rgb_0.png")) == 127).all()
    js = json.loads((out / "scene_render_metrics.json").read_text())
    assert set(js) == {"views", "psnr_mean", "ssim_mean"} and len(js["views"]) == 6 and all(set(v) == {"psnr", "ssim"} for v in js["views"])
    assert js["views"][3] == {"psnr": 23.0, "ssim": pytest.approx(0.7)} and js["psnr_mean"] == pytest.approx(22.5) and js["ssim_mean"] == pytest.approx(0.65)


def test_render_scene_image_rejects_block_counts_before_touching_a_device():
    rays = R.Rays(torch.zeros(4, 3), torch.tensor([[0.0, 0.0, 1.0]]).expand(4, 3))
    with pytest.raises(ValueError):
        R.render_scene_image([], rays)
    with pytest.raises(ValueError):
        R.render_scene_image([None] * 5, rays)
