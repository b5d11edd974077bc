"""Seeded inputs of the marching-cubes tests (tests/test_mc_host.py, tests/test_hip_marching_cubes.py).  Every lattice is float32 [nz, ny, nx]."""
import itertools

import numpy as np

# ---------------------------------------------------------------------------------------------- single configurations and neighbour pairings
def config_lattice(cfg, inside=1.0):
    """Configuration cfg (bit c: corner (c & 1, c >> 1 & 1, c >> 2 & 1) inside) as the 2^3 inner nodes of a 4^3 lattice whose shell is 0."""
    v = np.zeros((4, 4, 4), dtype=np.float32)
    for c in range(8):
        if cfg >> c & 1:
            v[1 + (c >> 2 & 1), 1 + (c >> 1 & 1), 1 + (c & 1)] = inside
    return v


def all_configs_lattice(seed=0):
    """All 256 configurations in ONE lattice [4, 64, 64]: configuration c fills the inner 2^3 nodes of the 4^3 footprint at (x, y) = 4 * (c % 16,
    c // 16); inside values drawn from {1, 3} by `seed`, outside 0."""
    rng = np.random.default_rng(seed)
    v = np.zeros((4, 64, 64), dtype=np.float32)
    for cfg in range(256):
        x0, y0 = 4 * (cfg % 16), 4 * (cfg // 16)
        for c in range(8):
            if cfg >> c & 1:
                v[1 + (c >> 2 & 1), y0 + 1 + (c >> 1 & 1), x0 + 1 + (c & 1)] = rng.choice([1.0, 3.0])
    return v


def neighbour_pairs_lattice(axis):
    """Every pairing of two configurations that are neighbours along `axis` (0 x, 1 y, 2 z): the two cells share four corners, so a pairing is
    one of the 2^12 sign patterns of a 3 x 2 x 2 node block.  Pattern p fills such a block inside its own footprint with a 0 shell; the 4096
    footprints tile a 64 x 64 array.  Returns the lattice (about 330k nodes)."""
    ext = [2, 2, 2]
    ext[axis] = 3                                            # nodes per axis of a block, (x, y, z)
    fp = [e + 2 for e in ext]
    v = np.zeros((fp[2], 64 * fp[1], 64 * fp[0]), dtype=np.float32)
    offs = list(itertools.product(range(ext[2]), range(ext[1]), range(ext[0])))      # (z, y, x) of the 12 block nodes
    for p in range(4096):
        x0, y0 = fp[0] * (p % 64), fp[1] * (p // 64)
        for b, (dz, dy, dx) in enumerate(offs):
            if p >> b & 1:
                v[1 + dz, y0 + 1 + dy, x0 + 1 + dx] = 1.0
    return v


def random_shell_lattice(seed, n=9, density=0.5):
    """n^3 lattice, inner nodes inside (values 1..3) with probability `density`, shell 0."""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, n, n), dtype=np.float32)
    v[1:-1, 1:-1, 1:-1] = (rng.random((n - 2,) * 3) < density) * rng.integers(1, 4, (n - 2,) * 3)
    return v


def sphere_lattice(n=17, radius=0.7):
    c = np.linspace(-1.0, 1.0, n)
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    return (radius * radius - (X * X + Y * Y + Z * Z)).astype(np.float32), (-1.0,) * 3, (2.0 / (n - 1),) * 3


def torus_lattice(n=25, major=0.6, minor=0.25):
    c = np.linspace(-1.0, 1.0, n)
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    return (minor * minor - ((np.sqrt(X * X + Y * Y) - major) ** 2 + Z * Z)).astype(np.float32), (-1.0,) * 3, (2.0 / (n - 1),) * 3


# ---------------------------------------------------------------------------------------------- device shapes
NX = (2, 3, 63, 64, 65, 129)                                 # one node pair, odd, one short of / exactly / one past a wave's 64 lanes, three x steps
NYZ = (2, 3, 5, 9)                                           # 9 = one past the 8 rows / planes a workgroup owns: two tiles
# the scan works on (y, z) rows in blocks of 4096: 65 * 64 = 4160 rows need two blocks and the carry between them; nx = 3 keeps it at 12,480 nodes
SCAN_SHAPE = (3, 65, 64)                                     # (nx, ny, nz)
ORIGIN = (-1.3, 0.7, 0.1)                                    # not dyadic: every vertex operation rounds
SPACING = (0.1, 0.3, 0.07)
LEVEL = 1.5


def integer_lattice(nx, ny, nz, seed):
    """Integers 0..4 (level 1.5 splits them 2 : 3), float32 [nz, ny, nx]."""
    rng = np.random.default_rng(seed + 1000003 * nx + 1009 * ny + nz)
    return rng.integers(0, 5, (nz, ny, nx)).astype(np.float32)


def cut_lattice(n=(21, 13, 11)):
    """A ball of radius 9 around a corner region of a [nz, ny, nx] = (11, 13, 21) lattice: the surface leaves through four lattice faces."""
    nx, ny, nz = n
    Z, Y, X = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (81.5 - ((X - 4.0) ** 2 + (Y - 3.0) ** 2 + (Z - 2.0) ** 2)).astype(np.float32)


def vertex_bound(dims, origin, spacing):
    """Bound on |fp32 vertex coordinate - exact| per axis, from the operations of the vertex rule, u = 2^-24, for an edge on a lattice of n nodes
    along the axis (dims = (nx, ny, nz); node index i <= n - 1, t in [0, 1]):
      a = fl(level - v_p), b = fl(v_q - v_p), t^ = fl(a / b): three roundings, |t^ - t| <= 3 u t (1 + 2 u) <= 3.01 u;
      s = fl(i + t^): |s - (i + t^)| <= u (i + 1);   p = fl(s * spacing): relative u;   x = fl(origin + p): relative u of x.
    |x^ - x| <= |spacing| (3.01 u + u n) + u |spacing| n + u max|x|  <=  u (|spacing| (2 n + 3.01) + max(|origin|, |origin + n spacing|)),
    widened by 1.01 for the second-order terms.  The two plain coordinates origin + fl(j * spacing) make two of these roundings and fit inside."""
    u = 2.0 ** -24
    return [1.01 * u * (abs(s) * (2 * n + 3.01) + max(abs(o), abs(o + n * s))) for n, o, s in zip(dims, origin, spacing)]
