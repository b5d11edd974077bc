"""CPU: the sample-list training path without a GPU.  The per-sample rule of tests/render_samples_restatement.py against torch
autograd through tests/render_train_restatement.composite on a general (non-flat) field, term by term and all together, each of seven
deliberate errors seen; the argument rejection of the two entry points of csrc/render_samples.hip; NGPTrainer's ValueError; the command-line
flags; SubjectImages' with_alpha."""
import functools
import math

import numpy as np
import pytest
import torch

import march_cases as C
import render_samples_restatement as RS
import render_train_restatement as RT
import test_march_args_host as A
from oracle import ngp_oracle as N

REL = 1e-4                    # tests/test_render_bwd_host.py's bound for the same comparison (restatement against autograd, both CPU references)
DENSITY_SCALE = 150.0         # the random field's sigma is ~0.4: scaled so that rays reach T_all < 1e-4 and kept samples that do not survive exist


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _general():
    """150 rays of the ragged grid's training set through a random non-flat field (the oracle's networks): per marched sample sigma and colour."""
    case = C.random_case("ragged", 0.02, "random")
    sel = np.arange(0, 4500, 30)
    o, d, jit = torch.from_numpy(case.o[sel]), torch.from_numpy(case.d[sel]), torch.from_numpy(case.jitter[sel])
    gen = torch.Generator().manual_seed(3)
    base = torch.empty(3072 + N.n_grid_params()).uniform_(-0.5, 0.5, generator=gen)
    base[:3072].uniform_(-0.3, 0.3, generator=gen)
    color = torch.empty(7168).uniform_(-0.3, 0.3, generator=gen)
    roi, scene, model = (torch.tensor(v, dtype=torch.float32) for v in (case.roi, case.scene, case.model))
    with torch.no_grad():
        tm, occ = RT.march(o, d, torch.from_numpy(case.binary), roi, scene, case.dt, jit)
        idx = torch.nonzero(occ)
        x = o[idx[:, 0]] + tm[idx[:, 0], idx[:, 1], None] * d[idx[:, 0]]
        sig, raw = N.query_density(x, model, base)
        col = N.query_rgb(d[idx[:, 0]], raw, color)
    R, S = tm.shape
    sigma = torch.zeros(R, S, dtype=torch.float64).index_put((idx[:, 0], idx[:, 1]), sig.reshape(-1).double() * DENSITY_SCALE)
    rgb_s = torch.zeros(R, S, 3, dtype=torch.float64).index_put((idx[:, 0], idx[:, 1]), col.double())
    coef = torch.randn(R, 5, generator=gen, dtype=torch.float64)
    return case, tm, occ, idx, sigma, rgb_s, coef


def _autograd(which):
    """(dL/dsigma, dL/dc at the kept samples, upstream gradients) of L = sum a . rgb + b opacity + c depth with random per-ray coefficients."""
    case, tm, occ, idx, sigma, rgb_s, coef = _general()
    sigma, rgb_s = sigma.clone().requires_grad_(True), rgb_s.clone().requires_grad_(True)
    rgb, opac, depth, surv = RT.composite(sigma, rgb_s, occ, tm.double(), case.dt, C.BKGD)
    g_rgb = coef[:, :3] if which in ("rgb", "all") else None
    g_op = coef[:, 3] if which in ("opacity", "all") else None
    g_dep = coef[:, 4] if which in ("depth", "all") else None
    loss = 0.0
    if g_rgb is not None:
        loss = loss + (rgb * g_rgb).sum()
    if g_op is not None:
        loss = loss + (opac * g_op).sum()
    if g_dep is not None:
        loss = loss + (depth * g_dep).sum()
    loss.backward()
    i, j = idx[:, 0], idx[:, 1]
    gc = rgb_s.grad[i, j].numpy() if rgb_s.grad is not None else np.zeros((len(i), 3))
    ups = tuple(None if g is None else g.numpy() for g in (g_rgb, g_op, g_dep))
    return sigma.grad[i, j].numpy(), gc, surv[i, j].numpy(), ups, (rgb.detach().numpy(), opac.detach().numpy(), depth.detach().numpy())


def _records():
    case, tm, occ, idx, sigma, rgb_s, _ = _general()
    i, j = idx[:, 0], idx[:, 1]
    alpha = 1.0 - np.exp(-sigma[i, j].numpy() * float(np.float32(case.dt)))
    return RS.records64(i.numpy(), tm[i, j].double().numpy(), alpha, rgb_s[i, j].numpy(), C.BKGD, tm.shape[0])


def _restated(which, mutate=None):
    """The rule's (dL/dsigma, dL/dc) over ALL kept samples (zeros at those that do not survive)."""
    rec = _records()
    _, _, _, ups, _ = _autograd(which)
    gs, gc, M, n = RS.sample_grads64(rec, *ups, _general()[0].dt, mutate=mutate)
    if mutate == "nonsurvivors":
        return gs, gc
    full, full_c = np.zeros(len(rec.surv)), np.zeros((len(rec.surv), 3))
    full[rec.kept], full_c[rec.kept] = gs, gc
    return full, full_c


def test_records_restate_the_forward():
    rec = _records()
    _, _, surv, _, (rgb, opac, depth) = _autograd("all")
    assert np.array_equal(rec.surv, surv) and int((~surv).sum()) > 100 and int(surv.sum()) > 500
    assert np.abs(rec.C - rgb).max() <= 1e-12 and np.abs(rec.O - opac).max() <= 1e-12 and np.abs(rec.D - depth).max() <= 1e-12
    for r in np.unique(rec.ray)[:50]:
        assert rec.ord[rec.ray == r].tolist() == list(range(int(rec.count[r])))
    assert np.allclose(rec.T_next, rec.T_k - rec.w, rtol=0, atol=1e-15)


@pytest.mark.parametrize("which", ["rgb", "opacity", "depth", "all"])
def test_rule_equals_autograd_on_a_general_field(which):
    ds, dc, surv, _, _ = _autograd(which)
    gs, gc = _restated(which)
    assert not ds[~surv].any() and not dc[~surv].any()                  # kept samples that do not survive get nothing
    r = _rel(gs, ds)
    print(f"{which}: dL/dsigma rel L2 {r:.3e} over {int(surv.sum())} survivors")
    assert r <= REL
    if which in ("rgb", "all"):
        rc = _rel(gc, dc)
        print(f"{which}: dL/dc rel L2 {rc:.3e}")
        assert rc <= REL
    else:
        assert not gc.any() and not dc.any()


@pytest.mark.parametrize("mutate", RS.MUTATIONS)
def test_every_planted_error_is_seen(mutate):
    """Each deliberate error moves dL/dsigma or dL/dc of the three-term loss beyond four times the bound.  The opacity term at kept samples
    that do not survive is dt g_O (1 - O) with 1 - O < 1e-4 (such samples exist only behind an early stop), far below the norm of the whole
    vector whatever the rule: that error is measured where it acts, with the opacity loss alone on the rays that stopped early, and it moves
    elements whose reference is exactly 0."""
    if mutate == "nonsurvivors":
        ds, _, surv, _, _ = _autograd("opacity")
        gs, _ = _restated("opacity", mutate)
        ray = _records().all_ray
        stopped = np.isin(ray, np.unique(ray[~surv]))
        r = _rel(gs[stopped], ds[stopped])
        print(f"mutation {mutate}: dL/dsigma rel L2 {r:.3e} on the {int(stopped.sum())} kept samples of rays that stopped early")
        assert not ds[~surv].any() and np.all(gs[~surv] != 0) and r > 4 * REL
        return
    ds, dc, _, _, _ = _autograd("all")
    gs, gc = _restated("all", mutate)
    r, rc = _rel(gs, ds), _rel(gc, dc)
    print(f"mutation {mutate}: dL/dsigma rel L2 {r:.3e}, dL/dc rel L2 {rc:.3e}")
    assert max(r, rc) > 4 * REL


# ------------------------------------------------------------------------------------------------------------------------ argument rejection
DEV = A.DEV


def _train_samples(lib, n, b, capacity=4, records=None):
    rec = [DEV] * 9 if records is None else records
    return lib.dreg_ngp_render_train_samples(DEV, DEV, DEV, n, *A._grid(b), b["table"], b["w1"], b["w2"], b["cw1"], b["cw2"], b["cw3"], *A._tail(b), 1e-4,
                                             A.V3, DEV, DEV, DEV, DEV, DEV, capacity, *rec, DEV, None)


def _grad(lib, n, **over):
    a = dict(ray=DEV, t=DEV, T=DEV, w=DEV, c=DEV, P=DEV, Pd=DEV, dirs_in=DEV, rgb=DEV, op=DEV, dep=DEV, g_rgb=None, g_op=None, g_dep=None, dt=0.01,
             dirs=DEV, gs=DEV, gc=DEV)
    a.update(over)
    return lib.dreg_ngp_samples_grad(n, a["ray"], a["t"], a["T"], a["w"], a["c"], a["P"], a["Pd"], a["dirs_in"], a["rgb"], a["op"], a["dep"],
                                     a["g_rgb"], a["g_op"], a["g_dep"], a["dt"], a["dirs"], a["gs"], a["gc"], None)


@pytest.mark.parametrize("case", [c for c, _, _ in A.BAD])
def test_train_samples_rejects_what_the_marchers_reject(case):
    from dreg_nerf_amd import lib as L
    lib = L.load()
    b = A._block(next(over for c, over, _ in A.BAD if c == case))
    assert _train_samples(lib, 0, b) == 0                               # no rays: DREG_OK, nothing examined
    assert _train_samples(lib, 1, b) == A.EINVAL


def test_train_samples_rejects_its_own_arguments():
    from dreg_nerf_amd import lib as L
    lib = L.load()
    b = A._block({})
    assert _train_samples(lib, 0, b, capacity=-1) == 0                  # no rays first
    assert _train_samples(lib, -1, b) == A.EINVAL
    assert _train_samples(lib, 1, b, capacity=-1) == A.EINVAL
    for k in range(9):
        rec = [DEV] * 9
        rec[k] = None
        assert _train_samples(lib, 0, b, capacity=4, records=rec) == 0
        assert _train_samples(lib, 1, b, capacity=4, records=rec) == A.EINVAL, k


def test_samples_grad_rejections_and_the_all_null_call():
    from dreg_nerf_amd import lib as L
    lib = L.load()
    assert _grad(lib, 0, ray=None, g_rgb=DEV) == 0                      # no records first
    assert _grad(lib, -1, g_rgb=DEV) == A.EINVAL
    for k in ("ray", "t", "T", "w", "c", "P", "Pd", "dirs_in", "rgb", "op", "dep", "dirs", "gs", "gc"):
        assert _grad(lib, 5, g_rgb=DEV, **{k: None}) == A.EINVAL, k
    assert _grad(lib, 5, g_rgb=DEV, dt=0.0) == A.EINVAL and _grad(lib, 5, g_rgb=DEV, dt=math.nan) == A.EINVAL
    assert _grad(lib, 5) == 0                                           # all three upstream gradients null: nothing is launched (the addresses are made up)


# ------------------------------------------------------------------------------------------------------------------------ the host layers
class _NoData:
    pass


def test_trainer_requires_the_sample_list_for_an_opacity_loss():
    from dreg_nerf_amd import ngp, ngp_train
    aabb = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    f = ngp.NGPradianceField(aabb)
    g = ngp.OccupancyGrid(aabb, 8)
    with pytest.raises(ValueError, match="samples"):
        ngp_train.NGPTrainer(f, g, _NoData(), aabb, 100, opacity_loss_weight=0.1)
    with pytest.raises(ValueError):
        ngp_train.NGPTrainer(f, g, _NoData(), aabb, 100, backward="rays", opacity_loss_weight=1e-3)
    with pytest.raises(ValueError):
        ngp_train.NGPTrainer(f, g, _NoData(), aabb, 100, backward="points")
    with pytest.raises(ValueError):
        ngp_train.NGPTrainer(f, g, _NoData(), aabb, 100, backward="samples", opacity_loss_weight=-1.0)
    t = ngp_train.NGPTrainer(f, g, _NoData(), aabb, 100)
    assert t.backward == "rays" and t.opacity_loss_weight == 0.0
    t = ngp_train.NGPTrainer(f, g, _NoData(), aabb, 100, backward="samples", opacity_loss_weight=0.1)
    assert t.backward == "samples" and t.opacity_loss_weight == 0.1
    t = ngp_train.NGPTrainer(f, g, _NoData(), aabb, 100, backward="rays", opacity_loss_weight=0.0)
    assert t.backward == "rays"


def test_render_image_train_rejects_an_unknown_backward():
    from dreg_nerf_amd import ngp_train
    with pytest.raises(ValueError):
        ngp_train.render_image_train(None, None, None, None, 0.01, backward="points")
    with pytest.raises(ValueError):
        ngp_train.render_image_train(None, None, None, None, 0.01, backward="samples", sample_capacity=-1)


def test_default_capacity():
    from dreg_nerf_amd import ngp_train
    aabb = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    dt = ngp_train.render_step_size_of(aabb)
    n_max = math.ceil(math.sqrt(27.0) / dt) + 2
    assert ngp_train.default_sample_capacity(3, aabb, dt) == 3 * n_max
    assert ngp_train.default_sample_capacity(4096, aabb, dt) == 1 << 20
    assert ngp_train.default_sample_capacity(0, aabb, dt) == 1


def test_command_line_flags():
    from dreg_nerf_amd.config import config_parser
    c = config_parser([])
    assert c.backward == "rays" and c.opacity_loss_weight == 0.0
    c = config_parser(["--backward", "samples", "--opacity_loss_weight", "0.05"])
    assert c.backward == "samples" and c.opacity_loss_weight == 0.05
    with pytest.raises(SystemExit):
        config_parser(["--backward", "points"])


def test_with_alpha_shapes_and_unchanged_defaults():
    from dreg_nerf_amd.nerf_images import SubjectImages
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (3, 6, 5, 4), dtype=np.uint8)
    images[0, :3, :, 3] = 0
    images[1, :, :, 3] = 255
    c2w = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    c2w[:, :3, 3] = rng.standard_normal((3, 3))
    s = SubjectImages(images, c2w, 7.0, "cpu")
    img, x, y = torch.tensor([0, 0, 1, 2]), torch.tensor([1, 4, 0, 3]), torch.tensor([0, 5, 2, 4])
    plain = s.rays_of(img, x, y)
    assert len(plain) == 2
    rays, pixels, alpha = s.rays_of(img, x, y, with_alpha=True)
    assert alpha.shape == (4,) and alpha.dtype == torch.float32 and pixels.shape == (4, 3)
    assert torch.equal(pixels, plain[1]) and torch.equal(rays.origins, plain[0].origins) and torch.equal(rays.viewdirs, plain[0].viewdirs)
    want = torch.from_numpy(images)[img, y, x, 3].float() / 255.0
    assert torch.equal(alpha, want) and float(alpha[0]) == 0.0 and float(alpha[2]) == 1.0
    assert torch.equal(pixels[0], torch.ones(3))                        # alpha 0: the white background
    g = lambda: torch.Generator().manual_seed(5)
    a = s.sample(16, generator=g())
    b = s.sample(16, generator=g(), with_alpha=True)
    assert len(a) == 2 and len(b) == 3 and b[2].shape == (16,)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].origins, b[0].origins)
    assert len(s.sample(16, generator=g(), with_alpha=False)) == 2
