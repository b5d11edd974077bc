"""GPU: the fused robust pose kernels (csrc/pose_ransac.hip, dreg_nerf_amd/pose_ransac.py) against the restatement of their rule
(tests/pose_ransac_restatement.py) on the seeded cases of tests/pose_ransac_cases.py: the exact lattice (bit for bit), random triplets (poses
within the counted fp32 bound, counts bit for bit at the kernel's own poses), the inlier kernel, the two-mode case end to end, determinism and the
C guards."""
import numpy as np
import pytest
import torch

import pose_ransac_cases as PC
import pose_ransac_restatement as PR
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import pose_ransac

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PATTERN = np.arange(12, dtype=np.float32) * np.float32(-1.25) + np.float32(7.5)


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def _launch(a, b, trip, thresh, pose=None, **kw):
    out = pose_ransac.ransac_launch(_dev(a), _dev(b), _dev(trip, torch.int32), thresh, pose=None if pose is None else _dev(pose), want_counts=True,
                                    want_poses=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


_EXACT = {}


def _exact(n):
    if n not in _EXACT:
        _EXACT[n] = PC.exact_points(n)
    return _EXACT[n]


@pytest.mark.parametrize("hyps", PC.EXACT_H)
@pytest.mark.parametrize("n", PC.EXACT_N)
def test_exact_lattice_bit_for_bit(n, hyps):
    """Lattice points, 90 degree rotations, dyadic translations and threshold, triplets with axis-aligned legs: every operation of the kernels is
    exact, so counts, best, pose and mask equal the fp64 restatement bit for bit: ties (the same triplets at many indices), invalid rows in every
    lane position (H = 4096), offsets at exactly thresh (inliers) and one ulp beyond (not)."""
    a, b, cls = _exact(n)
    trip = PC.exact_triplets(n, hyps)
    got = _launch(a, b, trip, PC.EXACT_THRESH, pose=PATTERN)
    want = PR.estimate(a, b, trip, PC.EXACT_THRESH, lo_iters=0, kernel_arithmetic=False)
    R, t, valid = PR.triad(a, b, trip, dtype=np.float64)
    print(f"N {n} H {hyps}: {int(valid.sum())} valid, best {want['best_index']} with {want['minimal_inliers']} inliers")
    assert np.array_equal(got["counts"], want["counts"].astype(np.int32))
    assert np.array_equal(got["poses"].astype(np.float64), np.concatenate([R.reshape(-1, 9), t], axis=1))
    assert got["status"][0] == want["status"] == 0 and got["best"].tolist() == [want["best_index"], want["minimal_inliers"]]
    assert np.array_equal(got["pose"].astype(np.float64), want["minimal_pose"])
    mask, count = PR.inliers(a, b, want["minimal_pose"], PC.EXACT_THRESH, np.float64)
    assert np.array_equal(got["mask"], mask) and count == want["minimal_inliers"]
    first = np.array_equal(got["pose"].astype(np.float64), PR.pose12_of(PC.EXACT_R1, PC.EXACT_T1))
    if first:
        assert got["mask"][(cls == PC.CLEAN1) | (cls == PC.AT_THRESH)].all() and not got["mask"][cls == PC.BEYOND].any()
    if hyps >= 63 and n >= 63:
        assert first and (want["scores"] == want["scores"].max()).sum() >= 2 and not valid[62]


@pytest.mark.parametrize("n,hyps", [(3, 1), (65, 65), (3000, 4096)])
def test_all_invalid_call_is_status_2_and_leaves_the_pose_untouched(n, hyps):
    a, b, _ = _exact(n)
    got = _launch(a, b, PC.exact_triplets(n, hyps, all_invalid=True), PC.EXACT_THRESH, pose=PATTERN)
    assert got["status"][0] == 2 and got["best"].tolist() == [-1, 0]
    assert got["pose"].tobytes() == PATTERN.tobytes()
    assert not got["counts"].any() and not got["poses"].any() and not got["mask"].any()


def test_fewer_than_three_correspondences_is_status_2():
    a, b, _ = _exact(3)
    got = _launch(a[:2], b[:2], np.array([[0, 1, 0], [1, 0, 2], [0, 1, 2]]), PC.EXACT_THRESH, pose=PATTERN)
    assert got["status"][0] == 2 and got["pose"].tobytes() == PATTERN.tobytes()
    pose, info = pose_ransac.estimate_pose(_dev(a[:2]), _dev(b[:2]), hyps=64)
    assert info["status"] == 2 and info["inliers"] == 0 and info["round_used"] == -1 and torch.equal(pose.cpu(), torch.eye(4)[:3])


@pytest.mark.parametrize("seed", PC.RANDOM_SEEDS)
def test_random_triplets(seed):
    """Per-hypothesis poses against the fp64 triad within the counted bound of pose_ransac_cases.triad_bound (c_R = 54 + 12 sqrt(2) (1 / sin_a +
    1 / sin_b) roundings of 2^-24 per entry of R) on the well-conditioned triplets; validity equal to the fp32 restatement's on ALL triplets; counts
    equal, bit for bit and without exclusions, to the fp32 restatement evaluated at the kernel's own output poses (the same operations)."""
    a, b, trip = PC.random_case(seed)
    got = _launch(a, b, trip, PC.RANDOM_THRESH)
    well, bR, bt = PC.triad_bound(a, b, trip)
    R64, t64, _ = PR.triad(a, b, trip, dtype=np.float64)
    _, _, v32 = PR.triad(a, b, trip, dtype=np.float32)
    Rk, tk = got["poses"][:, :9].reshape(-1, 3, 3), got["poses"][:, 9:]
    vk = got["poses"].any(axis=1)
    assert np.array_equal(vk, v32) and not vk[[5, 70, 200]].any()
    eR = np.abs(Rk.astype(np.float64) - R64).max(axis=(1, 2))
    et = np.abs(tk.astype(np.float64) - t64).max(axis=1)
    print(f"seed {seed}: {int(well.sum())} well-conditioned, largest |dR| / bound {float((eR / bR)[well].max()):.3f}, |dt| / bound {float((et / bt)[well].max()):.3f}")
    assert (eR[well] <= bR[well]).all() and (et[well] <= bt[well]).all()
    want = PR.scores(a, b, Rk, tk, vk, PC.RANDOM_THRESH, np.float32)
    assert np.array_equal(got["counts"], np.where(want < 0, 0, want).astype(np.int32))
    h, cnt, status = PR.select(want)
    assert got["best"].tolist() == [h, cnt] and got["status"][0] == status == 0 and cnt > 1500
    assert np.array_equal(got["pose"], got["poses"][h])
    mask, count = PR.inliers(a, b, got["pose"], PC.RANDOM_THRESH)
    assert np.array_equal(got["mask"], mask) and count == cnt


@pytest.mark.parametrize("n", [1, 64, 1025, 3000])
def test_pose_inliers_kernel(n):
    a, b, _ = PC.random_case(3)
    a, b = a[:n], b[:n]
    rng = np.random.default_rng(n)
    for pose in (np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), rng.normal(size=12), np.full(12, np.nan)):
        p32 = pose.astype(np.float32)
        mask, count = pose_ransac.pose_inliers(_dev(a), _dev(b), _dev(p32), 0.7)
        want_mask, want_count = PR.inliers(a, b, p32, 0.7)
        assert np.array_equal(mask.cpu().numpy(), want_mask) and int(count.item()) == want_count
    assert want_count == 0                                               # a NaN pose has no inliers


@pytest.mark.parametrize("sigma", [0.0, 0.005])
def test_two_mode_case_end_to_end(sigma):
    """Explicit triplets, minority 45 %, H = 4096, three refits.  The minimal stage equals the fp32 restatement's (index and count).  The final pose
    agrees with the restatement's to KABSCH_ATOL = 1e-5 per entry, the tolerance tests/test_hip_pointset_ops.py::test_small_ops_vs_golden holds
    the weighted Kabsch kernel to (the refits are that kernel, called as it is).  RRE / RTE against the planted motion stay within the host bounds
    widened by that tolerance: entries off by at most 1e-5 move the rotation by at most |dR|_F / sqrt(2) <= 3e-5 / sqrt(2) rad < degrees(3e-5)
    and the translation by at most sqrt(3) 1e-5 < 2e-5."""
    a, b, R, t, major = PC.two_mode_case(0.45, sigma, 0)
    trip = PC.draw_triplets(len(a), 4096, 0)
    want = PR.estimate(a, b, trip, PC.TWO_MODE_THRESH, kernel_arithmetic=True)
    pose, info = pose_ransac.estimate_pose(_dev(a), _dev(b), thresh=PC.TWO_MODE_THRESH, triplets=_dev(trip, torch.int32), lo_iters=3)
    p12 = torch.cat([pose[:, :3].reshape(9), pose[:, 3]]).cpu().numpy()
    rre, rte = PC.pose_errors(p12, R, t)
    rre_min, rte_min = PC.pose_errors(PR.pose12_of(info["minimal_pose"][:, :3].numpy(), info["minimal_pose"][:, 3].numpy()), R, t)
    print(f"sigma {sigma}: minimal pose index {info['best_index']} with {info['minimal_inliers']} inliers (RRE {rre_min:.3e} deg, RTE {rte_min:.3e}); "
          f"after the refits {info['round_inliers']} inliers, RRE {rre:.3e} deg, RTE {rte:.3e}; largest |pose - restatement| {np.abs(p12 - want['pose']).max():.3e}")
    assert info["status"] == 0 and info["best_index"] == want["best_index"] and info["minimal_inliers"] == want["minimal_inliers"]
    assert info["round_used"] == 2 and pose.dtype == torch.float32 and pose.shape == (3, 4) and pose.is_cuda
    assert np.abs(p12 - want["pose"].astype(np.float64)).max() <= PC.KABSCH_ATOL
    rre_b, rte_b = PC.TWO_MODE_BOUNDS[sigma]
    assert rre <= rre_b + np.degrees(3 * PC.KABSCH_ATOL) and rte <= rte_b + 2 * PC.KABSCH_ATOL
    assert info["inliers"] == info["round_inliers"][-1] and abs(info["inlier_ratio"] - info["inliers"] / len(a)) < 1e-12
    if sigma == 0:
        assert info["inliers"] >= major.sum()


def test_two_runs_are_bit_identical_and_equal_seeds_draw_equal_triplets():
    a, b, _, _, _ = PC.two_mode_case(0.40, 0.005, 2)
    A_, B_ = _dev(a), _dev(b)
    w = _dev(np.random.default_rng(0).uniform(0.2, 1.0, len(a)))
    runs = [pose_ransac.estimate_pose(A_, B_, w, thresh=PC.TWO_MODE_THRESH, hyps=1024, seed=5) for _ in range(2)]
    other = pose_ransac.estimate_pose(A_, B_, w, thresh=PC.TWO_MODE_THRESH, hyps=1024, seed=6)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1]["minimal_pose"], runs[1][1]["minimal_pose"])
    for k in ("status", "inliers", "best_index", "minimal_inliers", "round_inliers", "round_used"):
        assert runs[0][1][k] == runs[1][1][k]
    assert torch.equal(pose_ransac.draw_triplets(len(a), 1024, 5, DEV), pose_ransac.draw_triplets(len(a), 1024, 5, DEV))
    assert other[1]["best_index"] != runs[0][1]["best_index"] or not torch.equal(other[1]["minimal_pose"], runs[0][1]["minimal_pose"])
    trip = _dev(PC.draw_triplets(len(a), 1024, 0), torch.int32)
    x, y = (pose_ransac.ransac_launch(A_, B_, trip, PC.TWO_MODE_THRESH, want_counts=True, want_poses=True) for _ in range(2))
    torch.cuda.synchronize()
    assert all(torch.equal(x[k], y[k]) for k in ("best", "pose", "status", "mask", "counts", "poses"))


def test_c_guards():
    a, b, _ = _exact(65)
    A_, B_, T_ = _dev(a), _dev(b), _dev(PC.exact_triplets(65, 64), torch.int32)
    lib = L.load()
    nbytes = lib.dreg_pose_ransac_workspace_bytes(65, 64)
    assert nbytes >= 64 * 4 and lib.dreg_pose_ransac_workspace_bytes(65, 0) == 0 and lib.dreg_pose_ransac_workspace_bytes(-1, 64) == 0
    assert lib.dreg_pose_ransac_workspace_bytes(3000, 4096) // (4096 * 4) * 64 >= 256          # at least 256 workgroups at H = 4,096, N = 3,000
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    best, status = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    pose, mask = _dev(PATTERN), torch.zeros(65, dtype=torch.uint8, device=DEV)
    args = [L.ptr(A_), L.ptr(B_), 65, L.ptr(T_), 64, PC.EXACT_THRESH, 1e-4, L.ptr(ws), nbytes, L.ptr(best), L.ptr(pose), L.ptr(status), None, None, L.ptr(mask), L.stream()]

    def call(**change):
        names = ["a", "b", "N", "trip", "H", "thresh", "eps", "ws", "ws_bytes", "best", "pose", "status", "counts", "poses", "mask", "stream"]
        return lib.dreg_pose_ransac(*[change.get(k, v) for k, v in zip(names, args)])

    for k in ("a", "b", "trip", "ws", "best", "pose", "status"):
        assert call(**{k: None}) == -1
    assert call(H=0) == -1 and call(H=-5) == -1 and call(N=-1) == -1 and call(ws_bytes=nbytes - 4) == -1 and call(thresh=-1.0) == -1
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    inl = [L.ptr(A_), L.ptr(B_), 65, L.ptr(pose), PC.EXACT_THRESH, L.ptr(mask), L.ptr(count), L.stream()]
    for i in (0, 1, 3, 5, 6):
        assert lib.dreg_pose_inliers(*[None if j == i else v for j, v in enumerate(inl)]) == -1
    assert lib.dreg_pose_inliers(*inl[:2], -1, *inl[3:]) == -1
    torch.cuda.synchronize()
    assert pose.cpu().numpy().tobytes() == PATTERN.tobytes() and not mask.any()              # nothing was launched by the refused calls
    assert call() == 0 and call(mask=None) == 0
    torch.cuda.synchronize()
    assert status.item() == 0 and best[1].item() == mask.sum().item() > 0
