"""The density-with-gradient kernel (csrc/ngp_grad.hip, NGPradianceField.query_density_grad, ngp.field_normals) against the field's own forward (bit
for bit), the fp64 restatement of the gradient rule (tests/ngp_grad_restatement.py) within its counted roundings, the oracle's ReLU pattern, and a
planted linear field with a known gradient.  One CPU test pins the share of points the mask comparison leaves out."""
import ctypes
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import ngp_grad_restatement as GR
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import ngp
from oracle import ngp_oracle as NO

gpu = pytest.mark.gpu
AABB = [-1.0, -0.5, 0.0, 1.0, 1.5, 3.0]
SIZES = (1, 63, 64, 65, 257, 2000)
# fp32 roundings on the longest path from a term of the sum to grad_c in ngp_density_grad_kernel (products of two fp16 values are exact in fp32):
#   f_i = sum_j w1[j][i] g_j            64 additions
#   1 - w_a, 1 - w_b                     2     (w itself is shared with the restatement)
#   w_a * w_b                            1
#   f_2l t_0 + f_2l+1 t_1                2     (a product and the addition)
#   (w_a w_b) * v                        1
#   D_c += ...                           8     (corners)
#   scale_l * D_c                        1
#   du_c += ...                         16     (levels)
#   sigma * du_c, hi - lo, the division  3
C_ROUNDINGS = 64 + 2 + 1 + 2 + 1 + 8 + 1 + 16 + 3


@functools.lru_cache(maxsize=None)
def random_params():
    """mlp_base.params of a randomly initialised field with the hash table scaled up to +-0.5 (a fresh table's +-1e-4 would leave every hidden unit
    near zero), fp32 on the CPU."""
    f = ngp.NGPradianceField(AABB)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        f.mlp_base.params[3072:].uniform_(-0.5, 0.5, generator=g)
        f.mlp_base.params[:3072].uniform_(-0.3, 0.3, generator=g)
    return f.mlp_base.params.detach().clone()


def points(n, seed=0):
    """n points: mostly inside the aabb, one in 8 outside, one in 8 on a face (exactly)."""
    rng = np.random.default_rng(100 + n + seed)
    lo, hi = np.array(AABB[:3]), np.array(AABB[3:])
    x = lo + (hi - lo) * rng.uniform(0.001, 0.999, (n, 3))
    kind = rng.integers(0, 8, n)
    x[kind == 0] += (hi - lo) * rng.choice([-1.0, 1.0], (int((kind == 0).sum()), 3)) * 1.1
    face = np.nonzero(kind == 1)[0]
    ax = rng.integers(0, 3, len(face))
    x[face, ax] = np.where(rng.integers(0, 2, len(face)) == 0, lo[ax], hi[ax])
    if n == 1:
        x[0] = lo + (hi - lo) * 0.37
    return x.astype(np.float32)


def library_level_rows():
    """The level table the kernels are handed (dreg_ngp_level_table through NGPradianceField._levels) in the layout of oracle.level_table()."""
    (offset, size, res, scale, hashed), total = ngp._level_table()
    return [dict(offset=int(offset[l]), size=int(size[l]), res=int(res[l]), scale=float(scale[l]), hashed=bool(hashed[l])) for l in range(16)], total


def oracle_pre_activation(x):
    """The oracle's hidden pre-activations [N,64] (fp32 torch on the CPU, fp16-rounded inputs as oracle/ngp_oracle.py query_density forms them) of
    the SAME field as the kernel's.  The level scales are an input of the C ABI, not part of the arithmetic under test, so the oracle's encoding is
    evaluated on the table the kernel receives: oracle.level_table() forms the scales with numpy's exp2 / log2 and differs from the library's
    exp2f / log2f by one ulp at levels 3, 6, 8 and 11, which is a different field (one fp16 ulp in 3.5 % of the encoded values)."""
    p = random_params()
    aabb = torch.tensor(AABB)
    u = (torch.from_numpy(x) - aabb[:3]) / (aabb[3:] - aabb[:3])
    w1, _, table = NO.split_density_params(p)
    rows = library_level_rows()
    with mock.patch.object(NO, "level_table", lambda *a, **k: rows):
        enc = NO.hash_encode(u, NO.f16(table))
    return enc @ NO.f16(w1).T


def test_mask_comparison_leaves_out_at_most_half_a_percent():
    pre = oracle_pre_activation(points(2000))
    share = float((pre.abs() < 1e-5).float().mean())
    print(f"share of hidden units with |pre-activation| < 1e-5: {share:.5f}")
    assert share <= 0.005


@pytest.fixture(scope="module")
def field():
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        f.mlp_base.params.copy_(random_params())
    return f.to(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def host_copy(field):
    base16, _ = field._prepared()
    b = base16.cpu().numpy()
    return {"w1": b[:2048].reshape(64, 32), "w2": b[2048:3072].reshape(16, 64), "table": b[3072:].reshape(-1, 2), "lv": GR.levels_from_ctypes(field._levels),
            "aabb": np.array(AABB, dtype=np.float32)}


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_density_equals_the_forward_bit_for_bit_and_gradient_is_zero_outside(field, n):
    x = torch.from_numpy(points(n)).to(field.aabb.device)
    d, g = field.query_density_grad(x)
    d0, _ = field.query_raw(x)
    assert d.shape == (n, 1) and g.shape == (n, 3) and d.dtype == g.dtype == torch.float32
    assert torch.equal(d[:, 0], d0)
    lo, hi = field.aabb[:3], field.aabb[3:]
    inside = ((x > lo) & (x < hi)).all(dim=1)
    assert torch.equal(g[~inside], torch.zeros_like(g[~inside])) and torch.equal(d[~inside], torch.zeros_like(d[~inside]))
    if n >= 63:
        assert (~inside).sum() > 0 and inside.sum() > 0 and (d[inside] > 0).all() and (g[inside].abs().sum(dim=1) > 0).float().mean() > 0.9
    # a leading shape is kept
    if n == 64:
        d2, g2 = field.query_density_grad(x.view(4, 16, 3))
        assert d2.shape == (4, 16, 1) and g2.shape == (4, 16, 3) and torch.equal(g2.view(-1, 3), g)


@gpu
def test_gradient_within_the_counted_roundings_of_the_restatement(field, host_copy):
    """|grad - restatement| <= c 2^-24 M per component, the restatement given the kernel's own ReLU mask and density; M = the restatement's sum of the
    absolute values of its terms; c = C_ROUNDINGS, counted above from the kernel source (first order: c^2 2^-48 is far below the slack)."""
    x = points(2000, seed=1)
    xd = torch.from_numpy(x).to(field.aabb.device)
    d, g, m = field.query_density_grad(xd, return_mask=True)
    h = host_copy
    want, M = GR.density_grad(x, h["table"], h["w1"], h["w2"], h["lv"], h["aabb"], d[:, 0].cpu().numpy(), GR.mask_bits(m.cpu().numpy()))
    err = np.abs(g.cpu().numpy().astype(np.float64) - want)
    live = M > 0
    ratio = err[live] / (2.0 ** -24 * M[live])
    print(f"gradient vs fp64 restatement, {int(live.sum())} components: max |err| / (2^-24 M) = {ratio.max():.3f} (bound c = {C_ROUNDINGS}), "
          f"median {np.median(ratio):.3f}; median |grad| / M = {np.median(np.abs(want[live]) / M[live]):.3e}")
    assert live.mean() > 0.7 and np.all(err[~live] == 0.0)
    assert ratio.max() <= C_ROUNDINGS


@gpu
def test_relu_mask_agrees_with_the_oracle(field):
    """The kernel's mask (read back from the hidden activations the forward stored) against the oracle's h > 0 on the same level table, leaving out the
    units whose oracle pre-activation is within 1e-5 of zero: what remains between the two is the order of the fp32 sums of one 32-term dot product
    of terms below 0.15 (32 * 2^-24 * sum |terms| ~ 2e-6)."""
    x = points(2000)
    _, _, m = field.query_density_grad(torch.from_numpy(x).to(field.aabb.device), return_mask=True)
    bits = GR.mask_bits(m.cpu().numpy())
    pre = oracle_pre_activation(x).numpy()
    firm = np.abs(pre) >= 1e-5
    active = NO.f16(torch.relu(torch.from_numpy(pre))).numpy() > 0
    print(f"mask: {int(firm.sum())} of {firm.size} units compared, {int((bits != active)[firm].sum())} differ; {bits.mean():.3f} active")
    assert np.array_equal(bits[firm], active[firm]) and 0.2 < bits.mean() < 0.8


@gpu
def test_planted_linear_field_has_the_known_gradient():
    """Level 0 (dense, 16^3, scale 15) holds a c_x + b c_y + g c_z + d at corner c in feature 0, everything else is zero; W1 row 0 = e_0, W2[0][0] = 1:
    the logit is that linear function of 15 u + 1/2 wherever it is positive, so grad sigma = sigma 15 (a, b, g) / (hi - lo).
    The 1e-5 and the points: the derivative of a level is a DIFFERENCE of corner values, sum_corners +-(w_a w_b) v, whose absolute terms add up to
    about 2 v(x) against a result of one slope: its roundings are amplified by 2 v / slope.  Here f_0 = 1 and t_1 = 0 make v exact; the amplified
    roundings are 1 - w_a, 1 - w_b, w_a w_b, the product with v and 7 corner additions: 11; scale, sigma, hi - lo, the division and one level addition are
    5 more, unamplified.  With u in (0.01, 0.07) the position 15 u + 1/2 stays below 1.55 (two cells per axis, corners 0..2): v <= d + 1.55 (a + b + g)
    = 2.16 against the smallest slope 3/8, so |rel| <= 2^-24 (11 * 11.5 + 5) = 7.9e-6."""
    dev = torch.device("cuda", 0)
    a, b, g, d = 1 / 2, 3 / 8, 1 / 2, 1 / 32
    f = ngp.NGPradianceField(AABB)
    with torch.no_grad():
        p = f.mlp_base.params
        p.zero_()
        p[0] = 1.0                         # w1[0][0]
        p[2048] = 1.0                      # w2[0][0]
        c = torch.arange(16, dtype=torch.float32)
        val = a * c[None, None, :] + b * c[None, :, None] + g * c[:, None, None] + d          # [z][y][x]: entry x + 16 y + 256 z
        assert torch.equal(val.half().float(), val) and val.min() > 0
        p[3072:3072 + 2 * 4096:2] = val.reshape(-1)
    f = f.to(dev)
    rng = np.random.default_rng(5)
    lo, hi = np.array(AABB[:3]), np.array(AABB[3:])
    x = torch.from_numpy((lo + (hi - lo) * rng.uniform(0.01, 0.07, (1000, 3))).astype(np.float32)).to(dev)
    sig, grad = f.query_density_grad(x)
    assert torch.equal(sig[:, 0], f.query_raw(x)[0]) and (sig > 0).all()
    ext = torch.tensor(hi - lo, dtype=torch.float64)
    want = sig.double().cpu() * 15.0 * torch.tensor([a, b, g], dtype=torch.float64) / ext
    rel = ((grad.double().cpu() - want).abs() / want.abs()).max().item()
    print(f"planted field: max relative error of the gradient {rel:.2e}")
    assert rel <= 1e-5
    n = ngp.field_normals(f, x).cpu()
    dirn = -torch.tensor([a, b, g], dtype=torch.float64) / ext
    assert (n.double() - dirn / dirn.norm()).abs().max() <= 1e-5


@gpu
def test_field_normals_are_unit_or_exactly_zero(field):
    x = torch.from_numpy(points(2000, seed=2)).to(field.aabb.device)
    n = ngp.field_normals(field, x)
    _, g = field.query_density_grad(x)
    norm = n.norm(dim=1)
    zero = (n == 0).all(dim=1)
    assert n.shape == (2000, 3) and ((norm - 1).abs() < 1e-6)[~zero].all() and torch.equal(zero, (g == 0).all(dim=1)) and 0 < zero.sum() < 1000
    assert ((n * g).sum(dim=1)[~zero] < 0).all()                       # against the gradient: out of the surface


@gpu
def test_unbounded_field_raises_and_the_library_guards_its_arguments(field):
    u = ngp.NGPradianceField.from_inference_copies(AABB, True, *field._prepared(), field.aabb.device)
    with pytest.raises(NotImplementedError):
        u.query_density_grad(torch.zeros(4, 3, device=field.aabb.device))
    lib = L.load()
    base16, _ = field._prepared()
    x = torch.zeros(4, 3, device=base16.device)
    d, g = torch.full((4,), -7.0, device=base16.device), torch.full((4, 3), -7.0, device=base16.device)
    aabb = (ctypes.c_float * 6)(*AABB)
    head = [L.ptr(x), base16.data_ptr() + 3072 * 2, base16.data_ptr(), base16.data_ptr() + 2048 * 2, L.ptr(d), L.ptr(g), None]

    def call(head, n, contract):
        return lib.dreg_ngp_density_grad(*head, *field._levels, aabb, n, contract, L.stream())

    assert call(head, 4, 1) == -1 and call(head, -1, 0) == -1
    assert call(head[:4] + [None] + head[5:], 4, 0) == -1 and call([None] + head[1:], 4, 0) == -1 and call(head[:1] + [None] + head[2:], 4, 0) == -1
    assert call(head, 0, 0) == 0
    torch.cuda.synchronize()
    assert (d == -7).all() and (g == -7).all()                         # nothing was launched
    assert call(head, 4, 0) == 0
    torch.cuda.synchronize()
    assert (d >= 0).all() and torch.isfinite(g).all()
