#!/usr/bin/env python3
"""Record what the convolution dispatch's host-only entry points answer over a shape sweep (no GPU needed: the library loads without one and
none of these calls launches): dreg_conv3d_igemm_variant / _workspace_bytes, dreg_conv3d_wgrad_variant / _splits / _workspace_bytes and
dreg_conv3d_wgrad_group_fill / dreg_linear_wgrad_group_fill.  tests/golden/conv_dispatch.json is this script's output for the build BEFORE the
dispatch rules were stated once (igemm_choose / wgrad_choose in csrc/conv.hip); tests/test_abi_and_ddp.py replays the sweep on the current build.

usage: python tools/make_conv_dispatch_golden.py [--lib path/to/libdreg_nerf_hip.so] [--out tests/golden/conv_dispatch.json]"""
import argparse
import ctypes
import itertools
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreg_nerf_amd import lib as L

PARAMS = {
    # dense sweep: B x D^3 volumes, stride 1, same-size, pad = ksz // 2
    "dense": {"B": [1, 2, 8], "D": [1, 4, 8, 16, 32, 64], "Cin": [64, 128, 256, 512, 1024], "Cout": [64, 128, 256, 512], "ksz": [1, 3]},
    # row lists (active sets) over a B = 8 volume: lengths on both sides of 16,384 and 65,536
    "rows": {"B": [8], "D": [32, 64], "CinCout": [[256, 256], [64, 256], [128, 128], [64, 64], [256, 512]], "ksz": [1, 3, 5],
             "nrows": [1000, 16383, 16384, 28000, 65535, 65536, 90000, 200000]},
    # linear layers (1^3 volumes, rows = batch) for dreg_linear_wgrad_group_fill
    "linear": {"rows": [100, 5000, 9856, 20000, 70000], "CinCout": [[256, 256], [256, 1024], [1024, 256], [256, 64], [64, 128]]},
    # [B, Di, Cin, Do, Cout, ksz, stride, pad]: shapes outside the direct-to-LDS rules (the stem) and the stride-2 data gradients' class convolutions
    "other": [[8, 128, 8, 64, 64, 5, 2, 2], [8, 32, 64, 16, 128, 3, 2, 1], [8, 8, 256, 8, 512, 2, 1, 0], [8, 16, 128, 16, 1024, 2, 1, 0]],
}
DESC_WORDS = 36          # dreg_wgrad_group_desc_bytes() / 4; words 0..5 are the three pointers


def dense_shapes():
    p = PARAMS["dense"]
    return list(itertools.product(p["B"], p["D"], p["Cin"], p["Cout"], p["ksz"]))


def row_cases():
    p = PARAMS["rows"]
    return [(B, D, cc[0], cc[1], k, n) for B, D, cc, k, n in itertools.product(p["B"], p["D"], p["CinCout"], p["ksz"], p["nrows"])]


def linear_cases():
    p = PARAMS["linear"]
    return [(r, cc[0], cc[1]) for r, cc in itertools.product(p["rows"], p["CinCout"])]


def load(path=None):
    lib = ctypes.CDLL(path or L.LIB_PATH)
    for name in ("dreg_conv3d_igemm_variant", "dreg_conv3d_igemm_workspace_bytes", "dreg_conv3d_wgrad_variant", "dreg_conv3d_wgrad_splits",
                 "dreg_conv3d_wgrad_workspace_bytes", "dreg_conv3d_wgrad_group_fill", "dreg_linear_wgrad_group_fill", "dreg_wgrad_group_desc_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    assert lib.dreg_wgrad_group_desc_bytes() == 4 * DESC_WORDS
    return lib


GROUP_FIELDS = ("rc", "variant", "nblocks", "tilesCol", "tiles", "nsplit", "vps", "crc32 of the descriptor, pointers masked")


def _group(call):
    """(return code, *variant, *nblocks, tilesCol, tiles, nsplit, vps, crc32 of the descriptor with its three pointers masked); zeros when refused."""
    desc = (ctypes.c_uint32 * DESC_WORDS)()
    var, nb = ctypes.c_int(0), ctypes.c_int(0)
    rc = call(desc, var, nb)          # the pointers are stored, never dereferenced
    if rc != 0:
        return [rc, 0, 0, 0, 0, 0, 0, 0]
    words = [0] * 6 + list(desc)[6:]
    return [rc, var.value, nb.value, words[28], words[29], words[30], words[31], zlib.crc32(b"".join(w.to_bytes(4, "little") for w in words))]


def collect(lib):
    """The sweep's answers as flat integer lists (fixed number of values per case, in the order of dense_shapes() / row_cases() / linear_cases())."""
    out = {"dense_wgrad": [], "dense_group": [], "dense_igemm": [], "rows": [], "linear_group": [], "other": []}
    big = 1 << 40
    for B, D, cin, cout, k in dense_shapes():
        pad = k // 2
        out["dense_wgrad"] += [lib.dreg_conv3d_wgrad_variant(B, D, D, D, cin, cout, k, 0, 0, 0), lib.dreg_conv3d_wgrad_variant(B, D, D, D, cin, cout, k, 0, 0, 1),
                               lib.dreg_conv3d_wgrad_splits(B, D, D, D, cin, cout, k, 0), lib.dreg_conv3d_wgrad_workspace_bytes(B, D, D, D, cin, cout, k, 0),
                               lib.dreg_conv3d_wgrad_splits(B, D, D, D, cin, cout, k, 1), lib.dreg_conv3d_wgrad_workspace_bytes(B, D, D, D, cin, cout, k, 1)]
        out["dense_group"] += _group(lambda d, v, n: lib.dreg_conv3d_wgrad_group_fill(d, 256, 512, 768, big, B, D, D, D, cin, D, D, D, cout, k, 1, pad, ctypes.byref(v), ctypes.byref(n)))
        geo = (B, D, D, D, cin, D, D, D, cout, k, 1, pad)
        # (transposed, has_ws, has_addend): forward and data-gradient forms with / without a split-K workspace and an addend; then fp32
        out["dense_igemm"] += [lib.dreg_conv3d_igemm_variant(*geo, t, 0, ws, add, 0) for t, ws, add in ((0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 1))]
        out["dense_igemm"] += [lib.dreg_conv3d_igemm_workspace_bytes(*geo, t, add, 0) for t, add in ((0, 0), (0, 1), (1, 0))]
        out["dense_igemm"] += [lib.dreg_conv3d_igemm_variant(*geo, 0, 0, 1, 0, 1), lib.dreg_conv3d_igemm_workspace_bytes(*geo, 0, 0, 1)]
    for B, D, cin, cout, k, n in row_cases():
        geo = (B, D, D, D, cin, D, D, D, cout, k, 1, k // 2)
        out["rows"] += [lib.dreg_conv3d_wgrad_variant(B, D, D, D, cin, cout, k, 1, n, 0),
                        lib.dreg_conv3d_igemm_variant(*geo, 0, n, 0, 0, 0), lib.dreg_conv3d_igemm_variant(*geo, 1, n, 0, 1, 0)]
    for rows, cin, cout in linear_cases():
        out["linear_group"] += _group(lambda d, v, n: lib.dreg_linear_wgrad_group_fill(d, 256, 512, 768, big, rows, cin, cout, ctypes.byref(v), ctypes.byref(n)))
    for B, Di, cin, Do, cout, k, s, pad in PARAMS["other"]:
        geo = (B, Di, Di, Di, cin, Do, Do, Do, cout, k, s, pad)
        out["other"] += [lib.dreg_conv3d_igemm_variant(*geo, 0, 0, 1, 0, 0), lib.dreg_conv3d_igemm_variant(*geo, 0, 30000, 0, 0, 0), lib.dreg_conv3d_igemm_variant(*geo, 0, 0, 1, 0, 1),
                         lib.dreg_conv3d_igemm_workspace_bytes(*geo, 0, 0, 0)]
    return out


def pack(lists):
    """Few distinct answers repeat over the sweep: a sorted table of the distinct values and, per list, indices into it."""
    values = sorted({v for l in lists.values() for v in l})
    index = {v: i for i, v in enumerate(values)}
    return {"values": values, **{k: [index[v] for v in l] for k, l in lists.items()}}


def unpack(doc):
    return {k: [doc["values"][i] for i in l] for k, l in doc.items() if k not in ("values", "params", "group_fields")}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "conv_dispatch.json"))
    a = ap.parse_args()
    doc = {"params": PARAMS, "group_fields": list(GROUP_FIELDS), **pack(collect(load(a.lib)))}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(a.out, os.path.getsize(a.out), "bytes")
