"""GPU: every convolution instantiation of csrc/conv.hip on the integer operands of tests/conv_exact_cases.py against fp64, EXACTLY.

Every product and every fp32 partial sum is an integer below 2^24 (tests/test_conv_exact_host.py), so whatever the tile, the split count,
the MFMA shape or the order of accumulation, an fp32 output equals the fp64 reference and a bf16 output equals its round-to-nearest-even.
There is no tolerance in this file: an indexing, padding, swizzle, split or epilogue mistake moves some output by at least 1.  Rows a launch
must not touch hold a sentinel beforehand; workspaces are filled with NaN, so a partial that was never written cannot pass for a zero."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import conv_exact_cases as C
from dreg_nerf_amd import lib as L
from dreg_nerf_amd import brick, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF, F32 = torch.bfloat16, torch.float32


def dev(t, dtype):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def call(lib, name, *a):
    L.check(getattr(lib, name)(*a, L.stream()), name)


class knobs:
    """the library a case runs on: the product, or the measurement build with the case's knobs set (put back on exit, also after a failure)"""

    def __init__(self, case):
        self.case, self.pr = case, None

    def __enter__(self):
        if not self.case.knobs:
            return L.load()
        self.pr = L.probe()
        self.pr.__enter__()
        try:
            for setter, value, default in self.case.knobs:
                self.pr.set(setter, value, default)
        except BaseException:
            self.pr.__exit__(None, None, None)
            raise
        return self.pr.lib

    def __exit__(self, *exc):
        if self.pr is not None:
            torch.cuda.synchronize()
            self.pr.__exit__(*exc)
        return False


def assert_exact(got, want, what):
    """got, want: device tensors of one shape and dtype whose last axis is the channel (weight gradients: [cout, cin * taps])"""
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    g2, w2 = got.reshape(-1, got.shape[-1]).float().cpu(), want.reshape(-1, want.shape[-1]).float().cpu()
    bad = ~(g2 == w2)
    first = [(int(r), int(ch), float(g2[r, ch]), float(w2[r, ch])) for r, ch in bad.nonzero()[:8].tolist()]
    rows_bad = bad.any(1).nonzero().flatten()
    pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} values differ, in {rows_bad.numel()} of {bad.shape[0]} rows (first {rows_bad[:6].tolist()}, "
                f"last {rows_bad[-3:].tolist()}); (row, channel, got, want): {first}")


def rounded(exact, dtype):
    """the value an exact kernel stores: fp32, or round-to-nearest-even bf16"""
    f = exact.float()
    assert torch.equal(f.double(), exact)
    return (f if dtype == F32 else f.bfloat16()).to(DEV)


def pack(lib, w, cin_pad, for_dgrad, dt):
    """torch-layout weight [cout, cin_real, k, k, k] (host, integers) -> the packed operand on the device"""
    cout, cin_real, k = w.shape[0], w.shape[1], w.shape[2]
    if for_dgrad == 2:
        n = (1 if k == 1 else 8) * cin_real * lib.dreg_conv3d_kpad(1 if k == 1 else 2, cout, dt)
    elif for_dgrad == 1:
        n = cin_real * lib.dreg_conv3d_kpad(k, cout, dt)
    else:
        n = cout * lib.dreg_conv3d_kpad(k, cin_pad, dt)
    wd = dev(w, F32)
    out = torch.full((n,), float("nan"), dtype=BF if dt == 0 else F32, device=DEV)
    call(lib, "dreg_pack_conv_weight", L.ptr(wd), L.ptr(out), cout, cin_real, cin_pad, k, for_dgrad, dt)
    return out


def row_occupancy(lib, c, o):
    inocc = o.get("inocc").to(DEV).contiguous()
    flags = torch.full((c.B, *c.dout[:2]), 255, dtype=torch.uint8, device=DEV)
    call(lib, "dreg_conv_row_occupancy", L.ptr(inocc), L.ptr(flags), c.B, c.din[0], c.din[1], c.dout[0], c.dout[1], c.k, c.s, c.p)
    want = C.row_occupancy_exact(c)
    assert 0 < int((want == 0).sum()) < want.numel()                  # some rows are skipped
    assert torch.equal(flags.cpu() != 0, want != 0)
    return flags


# ------------------------------------------------------------------------------------------------ forward / row lists / epilogues
@pytest.mark.parametrize("c", C.FWD, ids=lambda c: c.id)
def test_forward_exact(c):
    o = C.operands(c)
    edt = BF if c.dt == 0 else F32
    odt = F32 if (c.out_f32 or c.dt == 1) else BF
    want = C.fwd_exact(c)
    with knobs(c) as lib:
        assert C.variant_query(lib, c) == c.variant
        x = dev(o.get("x"), edt)
        wpk = pack(lib, o.get("w"), c.cin, 0, c.dt)
        bias = dev(o.get("bias"), F32) if c.bias else None
        add = dev(o.get("add_same" if c.addend == "same" else "add_up"), odt) if c.addend else None
        da = tuple(add.shape[1:4]) if c.addend else (0, 0, 0)
        same = int(c.addend == "same")
        out = torch.full((c.B, *c.dout, c.cout), C.SENTINEL, dtype=odt, device=DEV)
        geo = (c.B, *c.din, c.cin, *c.dout, c.cout, c.k, c.s, c.p)
        nws = lib.dreg_conv3d_igemm_workspace_bytes(*geo, 0, int(bool(c.addend)), c.dt) if c.ws and c.api != "rows" else 0
        assert (nws > 0) == (c.variant is not None and c.variant % 10 == 1)
        wsp = torch.full((nws // 4,), float("nan"), dtype=F32, device=DEV) if nws else None
        pre = (L.ptr(x), L.ptr(wpk), L.ptr(out), L.ptr(bias), L.ptr(add))
        if c.api == "fwd":
            call(lib, "dreg_conv3d_igemm_ws", *pre, *geo, 0, int(c.relu), *da, same, c.dt, int(c.out_f32 and c.dt == 0), L.ptr(wsp), nws)
            assert_exact(out, rounded(want, odt), c.name)
        elif c.api == "fwd_occ":
            flags = row_occupancy(lib, c, o)
            call(lib, "dreg_conv3d_igemm_occ", *pre, *geo, 0, int(c.relu), *da, same, c.dt, 0, L.ptr(wsp), nws, L.ptr(flags))
            assert not want[flags.cpu() == 0].any()                           # the flags promise exact zeros, and the reference has them
            assert_exact(out, rounded(want, odt), c.name)
        elif c.api == "rows":
            r = C.rows(c)
            rd = r.to(DEV) if len(r) else torch.zeros(1, dtype=torch.int32, device=DEV)
            call(lib, "dreg_conv3d_igemm_rows", *pre, L.ptr(rd), len(r), *geo, 0, int(c.relu), *da, same, int(c.out_f32))
            full = torch.full_like(want, C.SENTINEL)
            full.view(-1, c.cout)[r.long()] = want.view(-1, c.cout)[r.long()]
            keep = torch.ones(c.M, dtype=torch.bool)
            keep[r.long()] = False
            torch.cuda.synchronize()
            assert bool((out.view(-1, c.cout)[keep.to(DEV)] == C.SENTINEL).all()), "a row outside the list was written"
            assert_exact(out, rounded(full, odt), c.name)
        elif c.api == "bnstats":
            V = c.M // c.B
            part = torch.full((c.B, max(V // 128, 1), c.cout, 2), float("nan"), dtype=F32, device=DEV)
            rpc = ctypes.c_int(-1)
            call(lib, "dreg_conv3d_igemm_bnstats", *pre, *geo, int(c.relu), *da, same, L.ptr(wsp), nws, L.ptr(part), ctypes.addressof(rpc))
            assert_exact(out, rounded(want, odt), c.name)
            if nws:
                assert rpc.value == 0                                          # a split-K launch leaves no sums
            else:
                assert rpc.value == 128
                assert_exact(part, rounded(C.bn_sums_exact(c), F32), c.name + " (sums)")
        elif c.api == "defer":
            nsplit, slc = ctypes.c_int(-1), ctypes.c_size_t(0)
            call(lib, "dreg_conv3d_igemm_defer", *pre, *geo, 0, int(c.relu), *da, same, L.ptr(wsp), nws, None, ctypes.addressof(nsplit), ctypes.addressof(slc))
            torch.cuda.synchronize()
            assert nsplit.value > 1 and slc.value == c.M * c.cout and nsplit.value * slc.value * 4 == nws
            total = wsp.view(nsplit.value, c.M, c.cout).sum(0).view(c.B, *c.dout, c.cout)      # integers: exact in any order
            assert_exact(total, rounded(want, F32), c.name)
            assert bool((out == C.SENTINEL).all()), "a deferred launch must leave `out` alone"
        else:
            raise AssertionError(c.api)


# ------------------------------------------------------------------------------------------------ data gradients
@pytest.mark.parametrize("c", C.DGRAD, ids=lambda c: c.id)
def test_data_gradient_exact(c):
    o = C.operands(c)
    want = C.dgrad_exact(c)
    with knobs(c) as lib:
        assert C.variant_query(lib, c) == c.variant
        g = dev(o.get("g"), BF)
        if c.api == "dgrad":
            wpk = pack(lib, o.get("w"), c.cin, 1, 0)
            out = torch.full((c.B, *c.din, c.creal), C.SENTINEL, dtype=BF, device=DEV)
            geo = (c.B, *c.dout, c.cout, *c.din, c.creal, c.k, c.s, c.p)
            nws = lib.dreg_conv3d_igemm_workspace_bytes(*geo, 1, 0, 0)
            wsp = torch.full((nws // 4,), float("nan"), dtype=F32, device=DEV) if nws else None
            call(lib, "dreg_conv3d_igemm_ws", L.ptr(g), L.ptr(wpk), L.ptr(out), None, None, *geo, 1, 0, 0, 0, 0, 0, 0, 0, L.ptr(wsp), nws)
        else:
            assert c.creal == c.cin
            wpk = pack(lib, o.get("w"), c.cin, 2, 0)
            out = dev(o.get("din0"), BF) if c.acc else torch.full((c.B, *c.din, c.cin), C.SENTINEL, dtype=BF, device=DEV)
            call(lib, "dreg_conv3d_dgrad_s2_acc" if c.acc else "dreg_conv3d_dgrad_s2", L.ptr(g), L.ptr(wpk), L.ptr(out), c.B, *c.din, c.cin, *c.dout, c.cout, c.k, c.p)
        assert_exact(out, rounded(want, BF), c.name)


# ------------------------------------------------------------------------------------------------ weight gradients
def reduce_batched(lib, recs):
    """recs: (workspace, dw, smax, case, accumulate bits) of layers whose partials are in their workspaces -> ONE dreg_wgrad_reduce_batched"""
    table = np.zeros(len(recs), dtype=ops._REDUCE_DT)
    blocks = 0
    for i, (ws, dw, smax, c, accbits) in enumerate(recs):
        table[i] = (ws.data_ptr(), dw.data_ptr(), smax, c.cout, lib.dreg_conv3d_kpad(c.k, c.cin, 0), c.k ** 3, c.cin, c.creal, accbits, blocks)
        blocks += lib.dreg_wgrad_reduce_blocks(c.cout, c.creal, c.k, smax)
    td = torch.from_numpy(table.view(np.uint8)).to(DEV)
    call(lib, "dreg_wgrad_reduce_batched", L.ptr(td), len(recs), 0, blocks)
    torch.cuda.synchronize()


def wgrad_buffers(lib, c, o):
    edt = BF if c.dt == 0 else F32
    g, x = dev(o.get("g"), edt), dev(o.get("x"), edt)
    dw = dev(o.get("dw0"), F32) if c.acc else torch.full((c.cout, c.creal, c.k ** 3), C.SENTINEL, dtype=F32, device=DEV)
    nws = lib.dreg_conv3d_wgrad_workspace_bytes(c.B, *c.dout, c.cin, c.cout, c.k, c.dt)
    ws = torch.full((nws // 4,), float("nan"), dtype=F32, device=DEV)
    return g, x, dw, ws, nws


@pytest.mark.parametrize("c", C.WGRAD, ids=lambda c: c.id)
def test_weight_gradient_exact(c):
    o = C.operands(c)
    want = C.wgrad_exact(c)
    with knobs(c) as lib:
        assert C.variant_query(lib, c) == c.variant
        g, x, dw, ws, nws = wgrad_buffers(lib, c, o)
        geo = (c.B, *c.din, c.cin, c.creal, *c.dout, c.cout, c.k, c.s, c.p)
        r = C.rows(c).to(DEV) if c.nrows >= 0 else None
        if c.api == "wgrad":
            call(lib, "dreg_conv3d_wgrad", L.ptr(g), L.ptr(x), L.ptr(dw), L.ptr(ws), nws, *geo, int(c.acc), c.dt, c.use_tr)
        elif c.api == "wgrad_occ":
            flags = row_occupancy(lib, c, o)
            call(lib, "dreg_conv3d_wgrad_occ", L.ptr(g), L.ptr(x), L.ptr(dw), L.ptr(ws), nws, *geo, int(c.acc), c.dt, c.use_tr, L.ptr(flags))
        elif c.api == "wgrad_rows":
            call(lib, "dreg_conv3d_wgrad_rows", L.ptr(g), L.ptr(x), L.ptr(dw), L.ptr(ws), nws, L.ptr(r), len(r), *geo, int(c.acc))
        elif c.api == "wgrad_partials":
            smax = lib.dreg_conv3d_wgrad_splits(c.B, *c.dout, c.cin, c.cout, c.k, 0)
            call(lib, "dreg_conv3d_wgrad_partials", L.ptr(g), L.ptr(x), L.ptr(ws), nws, L.ptr(r), 0 if r is None else len(r), *geo, None)
            if r is not None:
                torch.cuda.synchronize()
                kpad = lib.dreg_conv3d_kpad(c.k, c.cin, 0)
                written = int(ws.view(torch.int32)[smax * c.cout * kpad].item())
                assert 1 <= written < smax                                      # the list is worth fewer slices than the dense volume
                assert bool(torch.isnan(ws[written * c.cout * kpad:smax * c.cout * kpad]).all())
            reduce_batched(lib, [(ws, dw, smax, c, int(c.acc) | (2 if r is not None else 0))])
        else:
            raise AssertionError(c.api)
        assert_exact(dw.view(c.cout, -1), rounded(want, F32).view(c.cout, -1), c.name)


@pytest.mark.parametrize("name,variant,cases", C.GROUPS, ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_grouped_weight_gradient_exact(name, variant, cases):
    """dreg_*_wgrad_group_fill per layer, ONE dreg_wgrad_group_launch over the layers' descriptors, ONE batched reduce"""
    lib = L.load()
    nb = lib.dreg_wgrad_group_desc_bytes()
    table, keep, recs, block0 = bytearray(), [], [], 0
    for c in cases:
        o = C.operands(c)
        g, x, dw, ws, nws = wgrad_buffers(lib, c, o)
        desc = (ctypes.c_uint8 * nb)()
        var, nblk = ctypes.c_int(0), ctypes.c_int(0)
        if c.linear:
            rc = lib.dreg_linear_wgrad_group_fill(desc, L.ptr(g), L.ptr(x), L.ptr(ws), nws, c.B, c.cin, c.cout, ctypes.byref(var), ctypes.byref(nblk))
        else:
            rc = lib.dreg_conv3d_wgrad_group_fill(desc, L.ptr(g), L.ptr(x), L.ptr(ws), nws, c.B, *c.din, c.cin, *c.dout, c.cout, c.k, c.s, c.p,
                                                  ctypes.byref(var), ctypes.byref(nblk))
        assert rc == 0 and var.value == variant and nblk.value > 0, (c.name, rc, var.value, nblk.value)
        d = bytearray(bytes(desc))
        struct.pack_into("<i", d, nb - 4, block0)              # block0, the descriptor's last int: exclusive prefix of the workgroup counts
        table += d
        block0 += nblk.value
        keep.append((g, x))
        recs.append((ws, dw, lib.dreg_conv3d_wgrad_splits(c.B, *c.dout, c.cin, c.cout, c.k, 0), c, 0))
    td = torch.frombuffer(table, dtype=torch.uint8).clone().to(DEV)
    call(lib, "dreg_wgrad_group_launch", L.ptr(td), len(cases), variant, block0)
    reduce_batched(lib, recs)
    for c, (ws, dw, smax, _, _) in zip(cases, recs):
        assert_exact(dw.view(c.cout, -1), rounded(C.wgrad_exact(c), F32).view(c.cout, -1), c.name)


# ------------------------------------------------------------------------------------------------ the halo and brick kernels
@pytest.mark.parametrize("c", C.HALO, ids=lambda c: c.id)
def test_halo_exact(c):
    """dreg_conv3_halo_n, forward (bias, addend) and through the flipped-tap pack as the data gradient of a cin -> cout layer"""
    lib = L.load()
    o = C.operands(c)
    tr = c.api == "halo_dgrad"
    red, nout = (c.cout, c.cin) if tr else (c.cin, c.cout)            # channels reduced over / written
    assert lib.dreg_conv3_halo_supported(c.B, *c.din, red, nout) == 1
    src = dev(o.get("g" if tr else "x"), BF)
    w = dev(o.get("w"), F32)
    pk = torch.full((lib.dreg_conv3_halo_pack_bytes_n(red, nout) // 2,), float("nan"), dtype=BF, device=DEV)
    call(lib, "dreg_pack_conv_weight_halo", L.ptr(w), L.ptr(pk), c.cout, c.cin, int(tr))
    bias = dev(o.get("bias"), F32) if c.bias else None
    add = dev(o.get("add_same" if c.addend == "same" else "add_up"), BF) if c.addend else None
    da = tuple(add.shape[1:4]) if c.addend else (0, 0, 0)
    out = torch.full((c.B, *c.din, nout), C.SENTINEL, dtype=BF, device=DEV)
    call(lib, "dreg_conv3_halo_n", L.ptr(src), L.ptr(pk), L.ptr(out), L.ptr(bias), L.ptr(add), c.B, *c.din, red, nout, *da, int(c.addend == "same"), 0)
    assert_exact(out, rounded(C.dgrad_exact(c) if tr else C.fwd_exact(c), BF), c.name)


@pytest.mark.parametrize("c", C.BRICK, ids=lambda c: c.id)
def test_brick_exact(c):
    """dreg_conv3_brick on the tiles of the case's row list; the other rows keep the sentinel"""
    o = C.operands(c)
    r = C.rows(c).long()
    flags = torch.zeros(c.M, dtype=torch.uint8)
    flags[r] = 1
    bt = brick.build(flags.view(c.B, *c.din).to(DEV), len(r))
    assert bt.nrows == len(r) and not bt.overflow
    x = dev(o.get("x"), BF)
    wpk = brick.pack_weight(dev(o.get("w"), F32), False)
    bias = dev(o.get("bias"), F32) if c.bias else None
    add = dev(o.get("add_up"), BF) if c.addend else None
    out = torch.full((c.B, *c.din, c.cout), C.SENTINEL, dtype=BF, device=DEV)
    brick.conv(x, wpk, out, bias, add, bt, c.cin, c.cout)
    want = C.fwd_exact(c)
    full = torch.full_like(want, C.SENTINEL)
    full.view(-1, c.cout)[r] = want.view(-1, c.cout)[r]
    assert_exact(out, rounded(full, BF), c.name)
