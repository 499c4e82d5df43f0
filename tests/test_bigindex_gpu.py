"""Past 2^31 elements and 4 GiB, every kernel family, both sides of each 32-bit limit (the table, the data and the reference:
tests/bigindex_cases.py; their self-checks: tests/test_bigindex_cases.py).

Per pass of a case: the kernel runs ONCE on the whole tensor, between red zones (tests/redzone.py); the kernel shiftnd_last_kernel()
names is the one the table intends; out / grad_x are then compared with the reference chunk by chunk over ALL of the tensor
(torch.equal on the device, one synchronisation per chunk; the chunks are drawn again from their seeds, which also shows the inputs
unchanged); the C oracle checks a few planes of the first and last sample and of the samples that hold element 2^31, element 2^32 and
byte 2^32.  grad_w: the fp64 fixed-order temporal kernels bit for bit against float32(the exact sum); the spatial kernels within the
project's bars (fp32 tables 1e-5 of the largest entry, 16-bit tables cases.gw16_tol).  Each pass prints one line (shape, bytes, marks,
kernel, seconds, grad_w error) for the record.

Row 3 has no fallback: the first shape beyond the limit is refused at the C ABI with nothing launched, and by the op with a message
that names the way out -- which the last two tests then take (the same values in channels-last memory)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import bigindex_cases as B
import redzone as RZ
from cases import gw16_tol
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GIB = 1 << 30
ZP, WZP = 9, 7            # the quantized cases' input zero point (the fill) and table zero point
SEED_X, SEED_G = 101, 202


@pytest.fixture()
def abi():
    from torchshifts import abi as A
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    A.set_path_policy(0)
    yield A
    A.set_path_policy(0)


def need(gib, what):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip("%s needs %.1f GiB of device memory, %.1f GiB are free" % (what, gib, free / GIB))


def release():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def guarded(shape, dt, layout):
    """problem shape [N, C, spatial ...] in `layout` -> (the guarded buffer, the view the library is handed)"""
    shape = tuple(int(s) for s in shape)
    if layout == "nchw":
        g = RZ.Guarded(shape, dt, DEV)
        return g, g.t
    if layout == "nhwc":
        g = RZ.Guarded(shape, dt, DEV, "channels_last")
        return g, g.t
    N, C, T, M = shape
    if layout == "segment":                       # memory order N, T, C, M
        g = RZ.Guarded((N, T, C, M), dt, DEV)
        return g, g.t.transpose(1, 2)
    assert layout == "frames"                     # memory order N, T, M, C
    g = RZ.Guarded((N, T, M, C), dt, DEV)
    return g, g.t.permute(0, 3, 1, 2)


def fill(view, case, seed, lo, hi):
    for i, a, e in B.chunks(case):
        view[a:e].copy_(B.draw(seed, i, (e - a,) + tuple(view.shape[1:]), view.dtype, DEV, lo, hi))


def same(view, a, e, want, what):
    got = view[a:e]
    assert got.shape == want.shape and got.dtype == want.dtype, what + (got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):                # (one synchronisation per chunk)
        raise AssertionError(what + ("samples %d:%d" % (a, e), RZ._first_difference(got, want)))


def zones_intact(buffers, what):
    if bool(torch.stack([g.dirty() for _, g in buffers]).any()):
        for name, g in buffers:
            g.assert_intact((name,) + what)


def channels_of(case, n):
    """a few channels of sample n for the C oracle: the specials, the last, and the planes that hold the marks (contiguous layouts)"""
    C, per, plane = case["shape"][1], B.sample_numel(case), int(np.prod(case["shape"][2:]))
    es = B.es_of(B.DTYPES[case["dt"]])
    cs = {0, 1, 2, 3, C - 1}
    for at in ((1 << 31), (1 << 32), (1 << 32) // es):
        if at // per == n:
            c = (at - n * per) // plane
            cs.update({c, min(c + 1, C - 1)})
    return sorted(c for c in cs if c < C)


def host(t):
    t = t.detach().cpu().contiguous()
    return (t if t.dtype in (B.F32, B.F64) or not t.dtype.is_floating_point else t.float()).numpy()


def lines(a):
    """[1, k, T, M] -> the 1-D problem [M, k, T]"""
    return np.ascontiguousarray(a[0].transpose(2, 0, 1))


def frames(l):
    return np.ascontiguousarray(l.transpose(1, 2, 0))[None]


def oracle_slices(case, kind, pad, active, table, xv, gv, outv, b):
    """the C oracle on planes of the marked samples against what the kernel wrote there"""
    temporal = case["family"].startswith("temporal")
    nd = 1 if temporal else len(case["shape"]) - 2
    for n in B.marked_samples(case):
        cs = channels_of(case, n)
        what = (case["id"], kind, "oracle", "sample", n, "channels", cs)
        got = host(outv[n:n + 1, cs])
        xs = None if xv is None else host(xv[n:n + 1, cs])
        gs = None if gv is None else host(gv[n:n + 1, cs])
        t = table[cs]
        if case["dt"] == "u8":
            wq = (t.reshape(len(cs), -1) + WZP).numpy()
            if temporal:
                wq = np.concatenate([wq, np.full_like(wq, WZP)], 1)
            if kind == "pool_forward":
                from test_pooled_gpu import quantized_pool_references
                want = quantized_pool_references(xs, wq - WZP + 128, ZP, pad, (2, 2), O.default_borders(xs), list(xs.shape))[0]   # (its table's zero point is 128)
            else:
                want = O.forward_q(xs, wq, WZP, ZP, pad)
            assert np.array_equal(got, want), what
            continue
        w32 = t.to(B.F32).reshape(len(cs), -1).numpy()
        if temporal:
            if kind == "forward":
                want = frames(O.forward(lines(xs), w32, pad, active))
            else:
                want = frames(O.backward(lines(gs), w32, lines(xs if xs is not None else gs), pad, active)[0])
        elif kind == "forward":
            want = O.forward(xs, w32, pad, active)
        elif kind == "pool_forward":
            want = O.forward_pooled(xs, w32, pad, active, 2)
        elif kind in ("pool_backward", "pool_backward_input"):
            like = np.zeros((1, len(cs)) + tuple(case["shape"][2:]), np.float32)
            want = O.backward_pooled(gs, w32, xs if xs is not None else like, pad, active, 2)[0]
        else:
            like = np.zeros((1, len(cs)) + tuple(case["shape"][2:]), np.float32)
            want = O.backward(gs, w32, xs if xs is not None else like, pad, active, b)[0]
        want = torch.from_numpy(want).to(B.DTYPES[case["dt"]]).float().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), what


def check_grad_w(case, kind, GW, gw64, what):
    """-> the record's text.  The fp64 fixed-order kernels: float32(the exact sum), narrowed, bit for bit; the spatial kernels: the
    project's bars for sums of this length"""
    wdt = B.DTYPES[case["wdt"]]
    got = GW.t
    if case["family"] == "temporal_learn":
        want = gw64.to(B.F32).to(wdt)
        assert torch.equal(got, want), what + ("grad_w", RZ._first_difference(got, want))
        return "bitwise"
    err = float((got.to(B.F64) - gw64).abs().max() / gw64.abs().max().clamp_min(1e-30))
    bar = 1e-5 if wdt == B.F32 else gw16_tol(torch.finfo(wdt).eps)
    print("BIGINDEX grad_w", what, "max|gw - gw64| / max|gw64| = %.3g (bar %.3g)" % (err, bar))
    assert err < bar, what + ("grad_w", err, bar)
    return "%.2g" % err


def kernel_for(kernels, pad):
    return kernels if isinstance(kernels, str) else kernels[pad]


def run_pass(abi, case, index):
    """one row of a case's passes: the tensors are allocated and drawn once, then the call runs once per padding of the row, each
    time on poisoned outputs, and is checked whole"""
    kind, pads, active, kernels = case["passes"][index]
    family, layout = case["family"], case["layout"]
    dt, wdt = B.DTYPES[case["dt"]], B.DTYPES[case["wdt"]]
    P = case["shape"]
    C = P[1]
    nd = len(P) - 2
    temporal = family.startswith("temporal")
    quant = dt == B.U8
    backward = kind in ("backward", "pool_backward")
    needs_x = kind in ("forward", "pool_forward") or backward
    needs_g = kind not in ("forward", "pool_forward")
    # shapes: the window (a cut is the fixed case's alone) and the pooled sizes
    b = None
    gshape = oshape = P
    if case["cut"] is not None:
        b, new = abi.check_borders(list(P), case["cut"], nd)
        gshape = tuple(new)
    if kind.startswith("pool"):
        pshape = tuple(P[:2]) + tuple(s // 2 for s in P[2:])
        if kind == "pool_forward":
            oshape = pshape
        else:
            gshape = pshape
    limit = 40 if B.nbytes(case) > 6 * GIB else 20
    peak = (B.nbytes(case) * ((1 if needs_x else 0) + (1 if needs_g else 0) + 1)) / GIB + 6
    assert peak <= limit, (case["id"], kind, peak)
    need(peak, "%s %s" % (case["id"], kind))
    torch.cuda.reset_peak_memory_stats()
    table = B.weights_of(case)
    t0 = time.perf_counter()
    for k, v in case["knobs"]:
        abi.set_tuning(k, v)
    buffers = []

    def make(name, shape, dtype, lay):
        g, v = guarded(shape, dtype, lay)
        buffers.append((name, g))
        return g, v

    X = G = None
    xv = gv = None
    if needs_x:
        X, xv = make("x", P, dt, layout)
        fill(xv, case, SEED_X, 0, 7)
    if needs_g:
        G, gv = make("grad", gshape, dt, layout)
        fill(gv, case, SEED_G, -7, 7)
    OUT, outv = make("grad_x" if needs_g else "out", P if needs_g else oshape, dt, layout)
    GW = WS = None
    # the table as the call takes it
    if quant:
        cols = table.reshape(C, -1) + WZP
        if temporal and layout == "segment":
            cols = torch.cat([cols, torch.full_like(cols, WZP)], 1)      # the unflagged 2-D call: no shift along the pixels
        elif temporal:
            cols = cols.reshape(C)
        wd = cols.to(torch.int32).to(DEV)
    elif family == "temporal_fixed":
        s = -table if kind == "gradx_negated" else table
        wd = (torch.stack([s, torch.zeros_like(s)], 1) if layout == "segment" else s).to(dt).to(DEV)
    elif kind in ("backward_input", "pool_backward_input"):
        wd = table.to(dt).to(DEV)                 # (the x == NULL forms take a table of the tensors' type)
    else:
        wd = table.to(wdt).to(DEV)
    W, _ = make("w", tuple(wd.shape), wd.dtype, "nchw")
    W.t.copy_(wd)
    flags = {}
    if temporal and not (family == "temporal_fixed" and layout == "segment"):
        flags = dict(shift_dim0=True)
        if family == "temporal_learn" and layout == "frames":
            flags["frames"] = True
    if backward:
        GW, _ = make("grad_w", tuple(wd.shape), wd.dtype, "nchw")
        nws = 16
        for pad in pads:                          # (exactly what the size functions return, the largest over the row's paddings)
            if kind == "pool_backward":
                nws = max(nws, abi.backward_pooled_workspace_bytes(xv, pad, active, 2))
            else:
                p = abi.problem(xv, pad, active, None, w=W.t, **flags)
                nws = max(nws, int(abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(p))))
        WS, _ = make("workspace", (nws,), torch.uint8, "nchw")
    elif kind == "backward_input":
        WS, _ = make("workspace", (max(wd.numel() * wd.element_size(), 16),), torch.uint8, "nchw")
    for _, g in buffers:
        g.paint(0x7B)
    torch.cuda.synchronize()
    t_fill = time.perf_counter() - t0
    w64 = table.to(DEV)
    try:
        for pad in pads:
            kernel = kernel_for(kernels, pad)
            what = (case["id"], kind, "pad", pad, "active", active)
            OUT.poison()
            if GW is not None:
                GW.poison()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if quant and kind == "pool_forward":
                abi.forward_quantized_pooled(xv, W.t, WZP, ZP, pad, 2, out=outv)
            elif quant:
                abi.forward_quantized(xv, W.t, WZP, ZP, pad, out=outv, **flags)
            elif kind == "forward":
                abi.forward(xv, W.t, pad, active, out=outv, **flags)
            elif kind == "gradx_negated":
                abi.forward(gv, W.t, pad, 0, out=outv, **flags)
            elif kind == "backward":
                abi.backward(gv, W.t, xv, pad, active, grad_x=outv, grad_w=GW.t, workspace=WS.t, **flags)
            elif kind == "backward_input":
                abi.backward_input(gv, W.t, P, pad, b, grad_x=outv, workspace=WS.t)
            elif kind == "pool_forward":
                abi.forward_pooled(xv, W.t, pad, active, 2, out=outv)
            elif kind == "pool_backward":
                abi.backward_pooled(gv, W.t, xv, pad, active, 2, grad_x=outv, grad_w=GW.t, workspace=WS.t)
            else:
                assert kind == "pool_backward_input", kind
                abi.backward_pooled_input(gv, W.t, P, pad, 2, grad_x=outv)
            name = abi.last_kernel()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert name == kernel, what + ("ran", name, "intended", kernel)
            zones_intact(buffers, what)
            # the whole tensor against the reference, chunk by chunk; the chunks' indices start at zero
            gw64 = None
            for i, a, e in B.chunks(case):
                xc = gc = None
                if needs_x:
                    xc = B.draw(SEED_X, i, (e - a,) + tuple(P[1:]), dt, DEV, 0, 7)
                    same(xv, a, e, xc, what + ("x is unchanged",))
                if needs_g:
                    gc = B.draw(SEED_G, i, (e - a,) + tuple(gshape[1:]), dt, DEV, -7, 7)
                    same(gv, a, e, gc, what + ("the gradient is unchanged",))
                part = None
                if quant:
                    if kind == "pool_forward":
                        want = B.pooled_forward_q(xc, w64, ZP, pad)
                    elif temporal:
                        want = B.temporal_forward_q(xc, w64, ZP, pad)
                    else:
                        want = B.shift_forward(xc, w64, pad, False, nd, fill=ZP)
                elif temporal:
                    if kind == "forward":
                        want = B.narrow(B.temporal_forward(xc, w64, pad, active), dt)
                    else:
                        gx, part = B.temporal_backward(gc, xc, w64, pad, active)
                        want = B.narrow(gx, dt)
                elif kind == "forward":
                    want = B.narrow(B.shift_forward(xc, w64, pad, active, nd), dt)
                elif kind == "pool_forward":
                    want = B.pooled_forward(xc, w64, pad, active, dt)
                elif kind in ("pool_backward", "pool_backward_input"):
                    gx, part = B.pooled_backward(gc, xc, w64, pad, active, dt)
                    want = B.narrow(gx, dt)
                else:
                    gx, part = B.shift_backward(gc, xc, w64, pad, active, nd, b, sizes=P[2:])
                    want = B.narrow(gx, dt)
                same(outv, a, e, want, what + ("grad_x" if needs_g else "out",))
                if part is not None:
                    gw64 = part if gw64 is None else gw64 + part
                del xc, gc, want, part
            gw_text = "-"
            if backward:
                gw_text = check_grad_w(case, kind, GW, gw64.reshape(GW.t.shape), what)
            oracle_slices(case, kind, pad, active, table, xv, gv, outv, b)
            zones_intact(buffers, what)
            t3 = time.perf_counter()
            print("BIGINDEX %s | %s pad %d active %d | %s %s | %d elements, %d bytes | past %s | %s | call %.3f s, check %.1f s | grad_w %s"
                  % (case["id"], kind, pad, active, case["dt"], "x".join(map(str, P)), B.numel(case), B.nbytes(case),
                     ", ".join(case["marks"]) or "nothing (the boundary shape)", name, t2 - t1, t3 - t2, gw_text))
    finally:
        for k, _ in case["knobs"]:
            abi.set_tuning(k, 0)
    used = torch.cuda.max_memory_allocated() / GIB
    print("BIGINDEX %s | %s | allocate and draw %.1f s | peak %.1f GiB" % (case["id"], kind, t_fill, used))
    assert used <= limit, (case["id"], kind, "peak GiB", used)
    del X, G, OUT, GW, WS, W, xv, gv, outv, buffers
    release()


@pytest.mark.parametrize("case_id,index", B.PASSES, ids=["%s-%d-%s-%s" % (i, k, B.BY_ID[i]["passes"][k][0], ("sparse", "active")[B.BY_ID[i]["passes"][k][2]]) for i, k in B.PASSES])
def test_whole_tensor(abi, case_id, index):
    try:
        run_pass(abi, B.BY_ID[case_id], index)
    finally:
        release()


# ---- row 3: no fallback under SHIFTND_SHIFT_DIM0 ----------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f16", "f32"])
def test_the_first_shape_beyond_the_tshift_limit_is_refused_at_the_c_abi(abi, dtn):
    """SHIFTND_ERR_INVALID_ARGUMENT from both entry points, 0 from the workspace query, nothing launched: every output keeps its poison"""
    dt = B.DTYPES[dtn]
    shape = B.DECLINED_TSHIFT[dtn]
    N, C, T, M = shape
    nb = N * C * T * M * B.es_of(dt)
    assert nb == 1 << 32
    need(4 * nb / GIB + 2, "the refused tshift call")        # x, out, grad_x and one copy of an output's bytes
    try:
        x = torch.empty((N, T, C, M), dtype=dt, device=DEV).transpose(1, 2)       # (never read: nothing may be launched)
        w = B.temporal_weights(C, T, 3).to(dt).to(DEV)
        (OUT, outv), (GX, gxv) = guarded(shape, dt, "segment"), guarded(shape, dt, "segment")
        GW, WS = RZ.Guarded((C,), dt, DEV), RZ.Guarded((4096,), torch.uint8, DEV)
        for active in (0, 1):
            p = abi.problem(x, 0, active, None, shift_dim0=True)
            assert abi.lib().shiftnd_backward_workspace_bytes(ctypes.byref(p)) == 0, (dtn, active)
            RZ.run_guarded(lambda: abi.forward(x, w, 0, active, out=outv, shift_dim0=True), [], [("out", OUT)], [None],
                           ("refused forward", dtn, active), patterns=(0x7B,), raises="invalid argument")
            RZ.run_guarded(lambda: abi.backward(x, w, x, 0, active, grad_x=gxv, grad_w=GW.t, workspace=WS.t, shift_dim0=True), [],
                           [("grad_x", GX), ("grad_w", GW), ("workspace", WS)], [None] * 3, ("refused backward", dtn, active),
                           patterns=(0x7B,), raises="invalid argument")
        del x, OUT, GX, GW, WS, outv, gxv
    finally:
        release()


def _clips(t, T):
    """[N*T, C, H, W] (contiguous or channels-last) -> the problem view [N, C, T, H*W]"""
    NT, C, H, W = t.shape
    if t.is_contiguous():
        return t.view(NT // T, T, C, H * W).transpose(1, 2)
    return t.permute(0, 2, 3, 1).view(NT // T, T, H * W, C).permute(0, 3, 1, 2)


def test_the_op_refuses_the_contiguous_tensor_and_serves_it_in_channels_last(abi):
    """torchshifts::temporal_shift_learnable on a contiguous HIP tensor of 4 GiB: a RuntimeError that names the limit and the way out,
    raised before anything is allocated; temporal_shift_learnable_cl on the same values in channels-last memory: the reference's bits"""
    ops = torch.ops.torchshifts
    N, C, T, M = B.DECLINED_TSHIFT["f16"]
    case = dict(shape=(N, C, T, M), dt="f16")
    dt, pad = B.F16, 3
    need(14, "the 4 GiB op call")
    try:
        w = B.temporal_weights(C, T, 3)
        wd = w.to(DEV)                                            # fp32 weights with the fp16 tensor
        x = torch.empty((N * T, C, 64, 64), dtype=dt, device=DEV)
        held = torch.cuda.memory_allocated()
        for active in (False, True):
            with pytest.raises(RuntimeError, match=r"temporal_shift_learnable.*2\^31 - 16 two-byte units \(4 GiB\).*channels-last.*"
                                                   r"memory_format=torch.preserve_format.*split the batch"):
                ops.temporal_shift_learnable(x, wd, T, pad, active)
            with pytest.raises(RuntimeError, match=r"2\^31 - 16 two-byte units"):
                ops._temporal_shift_learnable_backward(x, wd, x, T, pad, active)
        assert torch.cuda.memory_allocated() == held, "the refusal allocated"
        del x
        release()
        xcl = torch.empty((N * T, C, 64, 64), dtype=dt, device=DEV, memory_format=torch.channels_last)
        fill(_clips(xcl, T), case, SEED_X, 0, 7)
        out = ops.temporal_shift_learnable_cl(xcl, wd, T, pad, True)
        assert abi.last_kernel() == "frames_active_forward" and out.stride() == xcl.stride(), abi.last_kernel()
        outv, w64 = _clips(out, T), w.to(DEV)
        for i, a, e in B.chunks(case):
            xc = B.draw(SEED_X, i, (e - a, C, T, M), dt, DEV, 0, 7)
            same(outv, a, e, B.narrow(B.temporal_forward(xc, w64, pad, True), dt), ("temporal_shift_learnable_cl", "out"))
        del xcl, out, outv
    finally:
        release()
