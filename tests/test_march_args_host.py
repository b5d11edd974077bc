"""Argument rejection of the ray marchers' entry points (no GPU): every marcher fills its block through csrc/march.h's march_fill_block, so the
renderers, the training backward, the two-block renderer (either block) and the visibility entry points reject the same things — a null hash
table, an empty occupancy grid, a step that is 0 or NaN and, where a scene interval is marched, an aabb whose diagonal is more than 1e8 steps —
with DREG_EINVAL before anything is launched (a launch would return a hipError_t instead, or fault on the made-up device addresses).  With no
rays the same arguments are DREG_OK: nothing is examined."""
import ctypes
import math

import pytest

from dreg_nerf_amd import lib as L

EINVAL = -1
DEV = 0x10000                 # stands for a device buffer: no entry point reads through it on the host
_u16 = (ctypes.c_uint32 * 16)(*range(16))
_f16 = (ctypes.c_float * 16)(*[1.0] * 16)
LEVELS = [ctypes.addressof(_u16)] * 3 + [ctypes.addressof(_f16), ctypes.addressof(_u16)]
_unit = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
UNIT = ctypes.addressof(_unit)
_v3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
V3 = ctypes.addressof(_v3)

# (id, what the block is given instead, renderers only)
BAD = [("null_table", dict(table=None), False),
       ("rx_0", dict(rx=0), False), ("ry_0", dict(ry=0), False), ("rz_0", dict(rz=0), False),
       ("dt_0", dict(dt=0.0), False), ("dt_nan", dict(dt=math.nan), False),
       ("diagonal_over_1e8_steps", dict(dt=1e-9), True)]


def _block(over):
    b = dict(binary=DEV, rx=8, ry=8, rz=8, coarse=None, table=DEV, w1=DEV, w2=DEV, cw1=DEV, cw2=DEV, cw3=DEV, dt=0.01)
    b.update(over)
    return b


def _grid(b):
    return [b["binary"], b["rx"], b["ry"], b["rz"], b["coarse"]]


def _tail(b):
    return LEVELS + [UNIT, UNIT, UNIT, -math.inf, math.inf, b["dt"], 0.0]


def _render(lib, n, b, train=False):
    rays = [DEV, DEV] + ([DEV] if train else [])
    fn = lib.dreg_ngp_render_train if train else lib.dreg_ngp_render
    return fn(*rays, n, *_grid(b), b["table"], b["w1"], b["w2"], b["cw1"], b["cw2"], b["cw3"], *_tail(b), 1e-4, V3, DEV, DEV, DEV, DEV, DEV, None)


def _bwd(lib, n, b):
    nws = int(lib.dreg_ngp_render_bwd_workspace_bytes(max(n, 1)))
    return lib.dreg_ngp_render_bwd(DEV, DEV, DEV, n, *_grid(b), b["table"], DEV, *_tail(b), 1e-4, DEV, DEV, DEV, DEV, DEV, nws, None)


def _pair(lib, n, src, tgt):
    blk = lambda b: [DEV, DEV] + _grid(b) + [b["table"], b["w1"], b["w2"], b["cw1"], b["cw2"], b["cw3"]] + _tail(b) + [V3]
    return lib.dreg_ngp_render_pair(n, *blk(src), *blk(tgt), 4.0, 1e-4, V3, DEV, DEV, DEV, DEV, DEV, DEV, None)


def _vis_common(b, np_):
    return [DEV, DEV, b["binary"], DEV, b["table"], b["w1"], b["w2"], *LEVELS, UNIT, UNIT, UNIT, b["rx"], b["ry"], b["rz"], 1, np_, b["dt"], 0.5, 1e-4, 0.0]


def _vis_queue(lib, n, b):
    return lib.dreg_surface_visibility_queue(*_vis_common(b, n), DEV, b["coarse"], None)


def _vis_desc(lib, n, b):
    desc = ctypes.create_string_buffer(int(lib.dreg_surface_visibility_desc_bytes()))
    return lib.dreg_surface_visibility_fill_desc(ctypes.addressof(desc), *_vis_common(b, n), DEV, b["coarse"])


ENTRIES = {"render": (_render, True), "render_train": (lambda lib, n, b: _render(lib, n, b, train=True), True), "render_bwd": (_bwd, True),
           "pair_src": (lambda lib, n, b: _pair(lib, n, b, _block({})), True), "pair_tgt": (lambda lib, n, b: _pair(lib, n, _block({}), b), True),
           "visibility_queue": (_vis_queue, False), "visibility_fill_desc": (_vis_desc, False)}
CASES = [(e, c) for e, (_, renderer) in ENTRIES.items() for c, _, only_renderers in BAD if renderer or not only_renderers]


@pytest.mark.parametrize("entry,case", CASES, ids=[f"{e}-{c}" for e, c in CASES])
def test_rejected_before_any_launch(entry, case):
    lib = L.load()
    call = ENTRIES[entry][0]
    b = _block(next(over for c, over, _ in BAD if c == case))
    assert call(lib, 1, b) == EINVAL
    assert call(lib, 0, b) == 0              # no rays: DREG_OK, nothing examined
