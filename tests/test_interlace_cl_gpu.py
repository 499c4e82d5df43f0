"""Channels-last temporal interlacing on the GPU: SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE_FRAMES through the C ABI
(csrc/shiftnd_interlace_frames.hip) on permuted views of (N, T, M, C) buffers, under ONE packed table -- the [N, C] offsets followed
by the [N, T, C] scales -- and through torch.ops.torchshifts_interlace_cl and memory_format=torch.preserve_format of
temporal_interlace_func and TemporalInterlace.

The reference is tests/test_interlace_gpu.py::_clip_reference per clip (the oracle's 1-D evaluation times the scale) on
(N, T, C, M) copies of the values.  Shapes and offset tables are those of tests/test_per_clip_cl_gpu.py ("specials": every piece
mixed; "pieces", "groups8": every piece uniform; "runs", "groups3": a boundary inside a piece), the scales
tests/test_interlace_gpu.py::_exact_scales, which differ along n, t and c.  Cases added for this kernel pair:
    (1, 2, 3, 2056) fp16   257 16-byte pieces a row (the backward: 514 of 8 bytes): the second and third round of the piece loop
    (1, 2, 3, 2048) fp16   exactly 256 pieces a row in the forward: one row per step
    (1, 2, 3, 1024) fp32   exactly 256 pieces a row in both kernels
    (1, 33, 3, 8) fp16     T = 33: nothing is sized by T
T = 1 is (2, 1, 5, 8) fp32 of the degenerate cases.  The backward takes a workgroup's rows in rounds of two row steps; the ragged
cases with 196, 90 and 130 rows walk two and more rounds, where a scale record is added to by a later round.

Exact data: x and grad_out on eighths, offsets on quarters, scales from {0.5, 1, 2, -1, 0}: every product, blend and sum is exact in
fp32, so everything is compared bit for bit in all four dtypes.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_interlace_func, temporal_shift_learnable_per_clip_func

import redzone as RZ
from exact16_cases import FLOOR16, assert_bits, assert_ulp_close, round16
from test_interlace_gpu import _check_table, _clip_reference, _close, _exact_scales
from test_interlace_gpu import _run_interlace as _run_contiguous
from test_per_clip_cl_gpu import CASES as CLIP_CASES
from test_per_clip_cl_gpu import RECORDS, _run_cl, _same_bits, _table, _tables
from test_tshift_cl_gpu import _buffer, _channels_last_inputs, _eighths, _es, _id, _put, _run, _view, _weights, _whole, _wide

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts_interlace_cl
KEEP = torch.preserve_format
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
KW = dict(shift_dim0=True, interlace_frames=True)
FWD, FWD_R = "frames_interlace_forward", "frames_interlace_forward_ragged"
BWD, BWD_R = "frames_interlace_backward", "frames_interlace_backward_ragged"

ROUNDS = ((1, 2, 3, 2056), F16, 0)
ADDED = [ROUNDS, ((1, 2, 3, 2048), F16, 0), ((1, 2, 3, 1024), F32, 0), ((1, 33, 3, 8), F16, 0)]
CASES = CLIP_CASES + ADDED
CHUNKED = [((2, 8, 196, 64), F16, 0), RECORDS]
SWEEP = list(itertools.product(range(5), (0, 1)))


def _names(shape, dt, off):
    return (FWD, BWD) if _whole(shape, dt, off) else (FWD_R, BWD_R)


def _to_sm(a):
    """(N, T, M, C) -> (N, T, C, M), the buffers of tests/test_interlace_gpu.py"""
    return np.ascontiguousarray(np.moveaxis(a, -1, 2))


def _to_cl(a):
    return np.ascontiguousarray(np.moveaxis(a, 2, -1))


def _reference(x, go, w, s, pad, active, dt):
    """x, go: (N, T, M, C); w [N, C]; s [N, T, C] -> out, grad_x (N, T, M, C), grad_offsets [N, C], grad_scales [N, T, C] (fp64)"""
    xs, gs = _to_sm(x), _to_sm(go)
    clips = [_clip_reference(xs[n:n + 1], gs[n:n + 1], w[n], s[n], pad, active, dt) for n in range(x.shape[0])]
    out, gx = _to_cl(np.concatenate([c[0] for c in clips])), _to_cl(np.concatenate([c[1] for c in clips]))
    return out, gx, np.stack([c[2] for c in clips]), np.stack([c[3] for c in clips])


@functools.lru_cache(maxsize=32)
def _inputs(ci, kind, table, pad, active):
    """x, go (N, T, M, C), offsets [N, C], scales [N, T, C] of CASES[ci] -- fp64 arrays holding values of the case's dtype -- and the
    reference.  Computed once, shared, never written to."""
    shape, dt, _ = CASES[ci]
    N, T, C = shape[0], shape[1], shape[-1]
    rs = np.random.RandomState(9000 + 1000 * ci + 100 * _tables(shape, dt).index(table) + 10 * pad + active + (50000 if kind == "random" else 0))
    if kind == "exact":
        x, go, w, s = _eighths(rs, shape), _eighths(rs, shape), _table(rs, shape, dt, pad, table), _exact_scales(rs, N, T, C)
    else:
        narrow = (lambda a: torch.from_numpy(a).to(dt).double().numpy())
        x, go = narrow(rs.uniform(-1, 1, size=shape)), narrow(rs.uniform(-1, 1, size=shape))
        w, s = narrow(_table(rs, shape, dt, pad, table, quarters=False)), narrow(rs.uniform(-2, 2, size=(N, T, C)))
    ref = _reference(x, go, w, s, pad, active, dt)
    for a in (x, go, w, s) + ref:
        a.setflags(write=False)
    return (x, go, w, s) + ref


def _pack(w, s, dt):
    return torch.from_numpy(np.concatenate([np.asarray(w).reshape(-1), np.asarray(s).reshape(-1)])).to(dt).cuda()


def _run_ilf(shape, dt, off, x, go, w, s, pad, active, wdt=None):
    """the flagged forward and backward on (N, T, M, C) buffers -> out, grad_x, grad_offsets [N, C], grad_scales [N, T, C]; the kernel
    names and the path are asserted"""
    N, T, C = shape[0], shape[1], shape[-1]
    table = _pack(w, s, wdt or dt)
    xd, gd = _put(x, dt, off), _put(go, dt, off)
    out, gx = _buffer(shape, dt, off, fill=0xA5), _buffer(shape, dt, off, fill=0xA5)
    names = _names(shape, dt, off)
    abi.forward(_view(xd), table, pad, active, out=_view(out), **KW)
    assert abi.last_kernel() == names[0] and abi.last_path() == abi.PATH_CL, (shape, dt, off, active, abi.last_kernel())
    gt = torch.full_like(table, float("nan"))
    abi.backward(_view(gd), table, _view(xd), pad, active, grad_x=_view(gx), grad_w=gt, **KW)
    assert abi.last_kernel() == names[1] and abi.last_path() == abi.PATH_CL, (shape, dt, off, active, abi.last_kernel())
    goff, gsc = abi.unpack_interlace(gt, N, T, C)
    return out, gx, goff, gsc


# ---- 1. exact data -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_exact_data(ci):
    shape, dt, off = CASES[ci]
    for table, (pad, active) in itertools.product(_tables(shape, dt), SWEEP):
        what = (_id(CASES[ci]), table, "pad", pad, "active", active)
        x, go, w, s, want_out, want_gx, goff64, gsc64 = _inputs(ci, "exact", table, pad, active)
        out, gx, goff, gsc = _run_ilf(shape, dt, off, x, go, w, s, pad, active)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        if dt in (F32, F64):
            assert np.array_equal(_wide(goff).astype(np.float64), goff64), what + ("grad_offsets",)
            assert np.array_equal(_wide(gsc).astype(np.float64), gsc64), what + ("grad_scales",)
        else:
            assert_bits(_wide(goff), round16(goff64.astype(np.float32), dt), what + ("grad_offsets, the fp64 sum rounded once",))
            assert_bits(_wide(gsc), round16(gsc64.astype(np.float32), dt), what + ("grad_scales, the fp64 sum rounded once",))
            # fp32 tables with the 16-bit tensor: the same bits in out and grad_x, both gradients the sums themselves
            out2, gx2, goff2, gsc2 = _run_ilf(shape, dt, off, x, go, w, s, pad, active, wdt=F32)
            assert goff2.dtype == F32 and gsc2.dtype == F32, what
            assert torch.equal(out2, out) and torch.equal(gx2, gx), what + ("mixed out / grad_x",)
            assert np.array_equal(_wide(goff2).astype(np.float64), goff64), what + ("mixed grad_offsets",)
            assert np.array_equal(_wide(gsc2).astype(np.float64), gsc64), what + ("mixed grad_scales",)


# ---- 2. random data: the bounds of tests/test_interlace_gpu.py::test_random_data ----------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_random_data(ci):
    shape, dt, off = CASES[ci]
    for table, (pad, active) in itertools.product(_tables(shape, dt), SWEEP):
        what = (_id(CASES[ci]), table, "pad", pad, "active", active)
        x, go, w, s, want_out, want_gx, goff64, gsc64 = _inputs(ci, "random", table, pad, active)
        out, gx, goff, gsc = _run_ilf(shape, dt, off, x, go, w, s, pad, active)
        if dt in (F32, F64) or not active:
            assert_bits(_wide(out), want_out, what + ("out",))
            assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        else:
            assert_ulp_close(_wide(out), want_out, dt, FLOOR16, what + ("out",))
            assert_ulp_close(_wide(gx), want_gx, dt, FLOOR16, what + ("grad_x",))
        for n in range(shape[0]):
            _check_table(_wide(goff)[n], goff64[n], dt, what + ("grad_offsets", n))
            _check_table(_wide(gsc)[n].reshape(-1), gsc64[n].reshape(-1), dt, what + ("grad_scales", n))


# ---- 3. the contiguous kernels ---------------------------------------------------------------------------------------------------
def _ulps16(a, b):
    """the largest distance of two 16-bit tensors in units of the last place (the two zeros coincide)"""
    bits = (lambda t: t.contiguous().view(torch.int16).int())
    key = (lambda i: torch.where(i < 0, -(i & 0x7fff), i))
    return int((key(bits(a)) - key(bits(b))).abs().max())


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_the_bits_of_the_contiguous_kernels(ci):
    """out and grad_x carry the bits of tinterlace_forward / tinterlace_backward on (N, T, C, M) copies of the same data, byte for
    byte, the signs of the zeros included: both evaluate in fp32, scale after the lerp in a multiply of its own and round once to 16
    bits.  Random data, so that the roundings matter; four of the ten (padding, mode) pairs.

    ONE EXCEPTION, in tinterlace_forward and not in the kernels under test: `out` of an fp16 tensor whose contiguous PLANES are made
    of 2-byte pieces (M odd).  In that one body the compiler forms narrow(y * scale) with v_fma_mixlo_f16 under a +0 addend -- the
    exact product rounded once, and 0 * -s = +0 -- where every other body of that kernel, every body of the channels-last kernels,
    the fp32 / fp64 bodies and the composition round the product to fp32 first and give -0.  There the two results
    are both correctly rounded from values one fp32 rounding apart, so they differ by at most ONE fp16 ulp, which is asserted, with
    the count printed; grad_x is byte for byte there too.  Measured: (1, 2, 3, 2048) 3 of 196608 elements of out, the other cases
    of the exception none (signs of filled zeros aside)."""
    shape, dt, off = CASES[ci]
    two_byte_planes = dt == F16 and shape[2] % 2 == 1
    for table, (pad, active) in itertools.product(_tables(shape, dt), ((0, 0), (0, 1), (3, 1), (4, 0))):
        what = (_id(CASES[ci]), table, "pad", pad, "active", active)
        x, go, w, s = _inputs(ci, "random", table, pad, active)[:4]
        out, gx, _, _ = _run_ilf(shape, dt, off, x, go, w, s, pad, active)
        sm = _run_contiguous(_to_sm(x).shape, dt, 0, _to_sm(x), _to_sm(go), w, s, pad, active)
        assert sm[4].startswith("tinterlace_forward") and sm[5].startswith("tinterlace_backward"), what
        for name, mine, theirs in (("out", out, sm[0].movedim(2, -1).contiguous()), ("grad_x", gx, sm[1].movedim(2, -1).contiguous())):
            if name == "out" and two_byte_planes:
                assert sm[4] == "tinterlace_forward_ragged", what
                print(what, "out: elements that differ in value from the 2-byte-piece body:", int((mine != theirs).sum()), "of", mine.numel())
                assert _ulps16(mine, theirs) <= 1, what + (name, _ulps16(mine, theirs))
            else:
                assert _same_bits(mine, theirs), what + (name,)


def test_two_rounds_in_the_four_element_body():
    """(192, 2, 196, 64) fp16: 192 clips x 4 chunks meet the plan's grid target at two row steps of 16-byte pieces, 64 rows a
    workgroup; the kernel's 8-byte pieces make that four row steps of 16 rows, two ROUNDS -- the second adds to the scale records
    of the first -- in the whole-piece body of four elements, the one the production shapes run.  Exact data, everything bit for bit."""
    shape, dt = (192, 2, 196, 64), F16
    N, T, M, C = shape
    assert _plan_bytes(N, C, T, M, 2) == 4 * N * C * (1 + T) * 8      # four workgroups a clip: 64 rows each
    rs = np.random.RandomState(88)
    for table, (pad, active) in (("pieces", (0, 1)), ("specials", (3, 0)), ("specials", (0, 1))):
        what = (shape, table, "pad", pad, "active", active)
        x, go, w, s = _eighths(rs, shape), _eighths(rs, shape), _table(rs, shape, dt, pad, table), _exact_scales(rs, N, T, C)
        want_out, want_gx, goff64, gsc64 = _reference(x, go, w, s, pad, active, dt)
        out, gx, goff, gsc = _run_ilf(shape, dt, 0, x, go, w, s, pad, active, wdt=F32)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        assert np.array_equal(_wide(goff).astype(np.float64), goff64), what + ("grad_offsets",)
        assert np.array_equal(_wide(gsc).astype(np.float64), gsc64), what + ("grad_scales",)


# ---- 4. determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CHUNKED + [ROUNDS], ids=_id)
def test_both_gradient_tables_are_deterministic(case):
    ci = CASES.index(case)
    for active in (0, 1):
        x, go, w, s = _inputs(ci, "random", "specials", 0, active)[:4]
        a = _run_ilf(*case, x, go, w, s, 0, active)
        b = _run_ilf(*case, x, go, w, s, 0, active)
        for i in (2, 3):
            assert _same_bits(a[i].contiguous(), b[i].contiguous()), (case, active, i)


# ---- 5. red zones: both tensors of each pass, the packed table, the packed gradient and the workspace between painted zones ---------
def _plan_bytes(n, c, t, m, es):
    """the formula include/shiftnd_hip.h states"""
    pieces = -(-c * es // 16)
    rps = 256 // pieces if pieces < 256 else 1
    steps = 8
    while steps > 1 and n * -(-m // (rps * steps)) < 768:
        steps //= 2
    return -(-m // (rps * steps)) * n * c * (1 + t) * 8


GUARDED = [((2, 3, 5, 8), F16, 0), ((2, 3, 5, 24), F32, 0), ((2, 3, 5, 5), F16, 0), ((2, 3, 4, 3), F64, 0), ((3, 2, 300, 8), F32, 0)]


@pytest.mark.parametrize("shape,dt,off", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, off):
    N, T, M, C = shape
    rs = np.random.RandomState(82)
    dev = torch.device("cuda")
    for pad, active, table in itertools.product((0, 3), (0, 1), ("specials", "runs")):
        what = (shape, str(dt), "pad", pad, "active", active, table)
        x, go, w, s = _eighths(rs, shape), _eighths(rs, shape), _table(rs, shape, dt, pad, table), _exact_scales(rs, N, T, C)
        want_out, want_gx, goff64, gsc64 = _reference(x, go, w, s, pad, active, dt)
        as_dt = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt))
        X, OUT, G, GX = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(4))
        W, GW = RZ.Guarded((N * C + N * T * C,), dt, dev), RZ.Guarded((N * C + N * T * C,), dt, dev)
        ws_bytes = abi.backward_workspace(_view(X.t), pad, active, **KW).numel()
        assert ws_bytes == _plan_bytes(N, C, T, M, _es(dt)), what      # both partial sets, sized exactly
        WS = RZ.Guarded((ws_bytes,), torch.uint8, dev)

        def forward():
            abi.forward(_view(X.t), W.t, pad, active, out=_view(OUT.t), **KW)
            return abi.last_kernel()

        def backward():
            abi.backward(_view(G.t), W.t, _view(X.t), pad, active, grad_x=_view(GX.t), grad_w=GW.t, workspace=WS.t, **KW)
            return abi.last_kernel()

        table_t = _pack(w, s, dt).cpu()
        names = _names(shape, dt, off // _es(dt))
        assert RZ.run_guarded(forward, [("x", X, as_dt(x)), ("table", W, table_t)], [("out", OUT)], [as_dt(want_out)],
                              what + ("forward",)) == names[0]
        packed64 = np.concatenate([goff64.reshape(-1), gsc64.reshape(-1)])
        want_gt = as_dt(packed64) if dt in (F32, F64) else as_dt(packed64.astype(np.float32))
        assert RZ.run_guarded(backward, [("grad_out", G, as_dt(go)), ("x", X, as_dt(x)), ("table", W, table_t)],
                              [("grad_x", GX), ("grad_table", GW), ("workspace", WS)], [as_dt(want_gx), want_gt, None],
                              what + ("backward",)) == names[1]


# ---- 6. the neighbours ---------------------------------------------------------------------------------------------------------
def test_the_neighbours_keep_their_kernels():
    """the per-clip and the per-channel flagged channels-last calls on one case still report their own kernel names (_run_cl and _run
    assert them)"""
    shape, dt, off = (2, 3, 5, 8), F16, 0
    rs = np.random.RandomState(83)
    x, go = _eighths(rs, shape), _eighths(rs, shape)
    for active in (0, 1):
        _run_cl(shape, dt, off, x, go, _table(rs, shape, dt, 0, "specials"), 0, active)
        assert abi.last_kernel() == "frames_backward"
        _run(shape, dt, off, x, go, _weights(rs, 8, 3, 0, dt=dt), 0, active)
        assert abi.last_kernel() == "frames_backward"


# ---- 7. through the op -----------------------------------------------------------------------------------------------------------
def _flat_view(t, T):
    """a dense channels-last [N*T, C, ...] tensor -> its memory as an (N, T, M, C) buffer (a view)"""
    C = t.shape[1]
    v = t.permute(0, *range(2, t.dim()), 1).reshape(t.shape[0] // T, T, -1, C)
    assert v.data_ptr() == t.data_ptr() and v.is_contiguous()
    return v


@pytest.mark.parametrize("dt,wdt", [(F32, F32), (F64, F64), (F16, F16), (BF16, F32)], ids=lambda d: str(d).split(".")[-1])
def test_preserve_format_through_the_op(dt, wdt):
    """channels-last 3-, 4- and 5-D inputs: the input's strides, the C-ABI call's bits in everything, and the composition on the
    channels-last per-clip op -- fp32 / fp64: out and input.grad bit for bit, both tables within 1e-5 of the largest entry; 16-bit:
    the sparse shift's out bit for bit, the rest within 1 ulp + FLOOR16 of the composition evaluated in fp32"""
    rs = np.random.RandomState(84)
    for (x, T), pad, active in itertools.product(_channels_last_inputs(dt, rs), range(5), (False, True)):
        what = (tuple(x.shape), pad, active)
        N, C = x.shape[0] // T, x.shape[1]
        go = torch.from_numpy(rs.uniform(-1, 1, size=tuple(x.shape))).to(dt)
        w = torch.from_numpy(rs.uniform(-T - 1, T + 1, size=(N, C))).to(wdt)
        s = torch.from_numpy(rs.uniform(-2, 2, size=(N, T, C))).to(wdt)
        xg, wg, sg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
        go_cl = torch.empty_like(xg).copy_(go.cuda())
        assert xg.stride() == x.stride() and go_cl.stride() == x.stride()
        out = temporal_interlace_func(xg, wg, sg, T, pad, active, memory_format=KEEP)
        assert abi.last_kernel() in (FWD, FWD_R) and abi.last_path() == abi.PATH_CL and out.stride() == xg.stride(), what
        gx, gw, gs = torch.autograd.grad(out, (xg, wg, sg), go_cl)
        assert gx.stride() == go_cl.stride() and gw.shape == w.shape and gs.shape == s.shape and gw.dtype == wdt and gs.dtype == wdt, what
        # (autograd ran the backward on its own thread; the kernel names are per thread: the same call from this one)
        gx_op, gw_op, gs_op = OPS._temporal_interlace_cl_backward(go_cl, wg.detach(), sg.detach(), xg.detach(), T, pad, active)
        assert abi.last_kernel() in (BWD, BWD_R) and gx_op.stride() == go_cl.stride(), what
        assert torch.equal(gx_op, gx) and torch.equal(gw_op, gw) and torch.equal(gs_op, gs), what
        # the C ABI on the same memory
        table = abi.pack_interlace(wg.detach(), sg.detach())
        d_out, d_gx, d_gt = torch.empty_like(xg), torch.empty_like(xg), torch.empty_like(table)
        abi.forward(_view(_flat_view(xg.detach(), T)), table, pad, active, out=_view(_flat_view(d_out, T)), **KW)
        abi.backward(_view(_flat_view(go_cl, T)), table, _view(_flat_view(xg.detach(), T)), pad, active, grad_x=_view(_flat_view(d_gx, T)),
                     grad_w=d_gt, **KW)
        d_goff, d_gsc = abi.unpack_interlace(d_gt, N, T, C)
        assert _same_bits(out.detach(), d_out) and _same_bits(gx, d_gx), what + ("against the C ABI",)
        assert torch.equal(gw, d_goff) and torch.equal(gs, d_gsc), what + ("tables against the C ABI",)
        # a contiguous gradient with the channels-last input: the plain route's contiguous grad_x, the same values
        gx2 = OPS._temporal_interlace_cl_backward(go.cuda(), wg.detach(), sg.detach(), xg.detach(), T, pad, active)[0]
        assert abi.last_kernel().startswith("tinterlace_backward") and gx2.is_contiguous() and torch.equal(gx2, gx), what
        # the default-format call: the same values, contiguous
        plain = temporal_interlace_func(xg.detach(), wg.detach(), sg.detach(), T, pad, active)
        assert abi.last_kernel().startswith("tinterlace_forward") and plain.is_contiguous() and torch.equal(plain, out.detach()), what
        # the composition on the channels-last per-clip op
        cdt = dt if dt in (F32, F64) else F32
        xc, wc, sc = (t.detach().to(cdt).clone(memory_format=KEEP).requires_grad_(True) for t in (xg, wg, sg))
        ref = temporal_shift_learnable_per_clip_func(xc, wc, T, pad, active, memory_format=KEEP) * sc.reshape((x.shape[0], C) + (1,) * (x.dim() - 2))
        rx, rw, rs_ = torch.autograd.grad(ref, (xc, wc, sc), go_cl.to(cdt))
        if dt in (F32, F64):
            assert torch.equal(out.detach(), ref.detach()), what + ("out against the composition",)
            assert torch.equal(gx, rx), what + ("input.grad against the composition",)
            _close(gw, rw, what + ("offsets.grad",))
            _close(gs, rs_, what + ("scales.grad",))
        else:
            want_out, want_gx = round16(_wide(ref), dt), round16(_wide(rx), dt)
            if not active:
                assert_bits(_wide(out), want_out, what + ("out",))
                assert_bits(_wide(gx), want_gx, what + ("input.grad",))
            else:
                assert_ulp_close(_wide(out), want_out, dt, FLOOR16, what + ("out",))
                assert_ulp_close(_wide(gx), want_gx, dt, FLOOR16, what + ("input.grad",))
            for n in range(N):
                _check_table(_wide(gw)[n], rw[n].double().cpu().numpy(), dt if wdt == dt else F32, what + ("offsets.grad", n))
                _check_table(_wide(gs)[n].reshape(-1), rs_[n].double().cpu().numpy().reshape(-1), dt if wdt == dt else F32, what + ("scales.grad", n))


def test_other_inputs_give_exactly_the_default_result():
    """a contiguous input and a view that is not dense: the plain route, contiguous results"""
    rs = np.random.RandomState(85)
    T = 3
    base = torch.from_numpy(rs.uniform(-1, 1, size=(6, 8, 4, 10))).float().cuda()
    for x0 in (base[..., :5].contiguous(), base.contiguous(memory_format=torch.channels_last)[..., ::2]):
        w0 = torch.from_numpy(rs.uniform(-T - 1, T + 1, size=(2, 8))).float().cuda()
        s0 = torch.from_numpy(rs.uniform(-2, 2, size=(2, T, 8))).float().cuda()
        go = torch.randn(6, 8, 4, 5, device="cuda")
        res = []
        for fmt in (torch.contiguous_format, KEEP):
            x, w, s = x0.detach().requires_grad_(True), w0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
            out = temporal_interlace_func(x, w, s, T, 0, True, memory_format=fmt)
            assert abi.last_kernel().startswith("tinterlace_forward") and out.is_contiguous()
            res.append((out.detach(),) + torch.autograd.grad(out, (x, w, s), go))
        assert res[0][1].is_contiguous() and res[1][1].is_contiguous()
        for a, b in zip(*res):
            assert torch.equal(a, b)


def test_a_group_table():
    rs = np.random.RandomState(86)
    shape, T, G = (6, 8, 7, 7), 3, 4
    N, C = shape[0] // T, shape[1]
    x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float().cuda().contiguous(memory_format=torch.channels_last)
    go = torch.empty_like(x).copy_(torch.from_numpy(rs.uniform(-1, 1, size=shape)).float().cuda())
    w = torch.from_numpy(rs.uniform(-T - 1, T + 1, size=(N, G))).float().cuda()
    s = torch.from_numpy(rs.uniform(-2, 2, size=(N, T, G))).float().cuda()
    for active in (False, True):
        wa, sa = w.clone().requires_grad_(True), s.clone().requires_grad_(True)
        wb, sb = w.repeat_interleave(C // G, dim=1).requires_grad_(True), s.repeat_interleave(C // G, dim=2).requires_grad_(True)
        xa, xb = x.clone(memory_format=KEEP).requires_grad_(True), x.clone(memory_format=KEEP).requires_grad_(True)
        out, ref = temporal_interlace_func(xa, wa, sa, T, 0, active, KEEP), temporal_interlace_func(xb, wb, sb, T, 0, active, KEEP)
        assert abi.last_kernel() == FWD and out.stride() == x.stride()
        out.backward(go)
        ref.backward(go)
        assert torch.equal(out, ref) and torch.equal(xa.grad, xb.grad)
        assert wa.grad.shape == (N, G) and torch.equal(wa.grad, wb.grad.view(N, G, C // G).sum(2))
        assert sa.grad.shape == (N, T, G) and torch.equal(sa.grad, sb.grad.view(N, T, G, C // G).sum(3))


def test_autocast_gives_fp32_gradients():
    """16-bit activations with fp32 tables, what torch.autocast hands the op: SHIFTND_WEIGHTS_F32, both table gradients fp32"""
    rs = np.random.RandomState(87)
    shape, T = (6, 8, 4, 5), 3
    for dt in (F16, BF16):
        x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt).cuda().contiguous(memory_format=torch.channels_last)
        go = torch.empty_like(x).copy_(torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt).cuda())
        w = torch.from_numpy(rs.uniform(-T - 1, T + 1, size=(2, 8))).float().cuda()
        s = torch.from_numpy(rs.uniform(-2, 2, size=(2, T, 8))).float().cuda()
        xg, wg, sg = x.clone(memory_format=KEEP).requires_grad_(True), w.clone().requires_grad_(True), s.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dt):
            out = temporal_interlace_func(xg, wg, sg, T, 0, True, memory_format=KEEP)
        assert abi.last_kernel() == FWD and out.stride() == x.stride()
        out.backward(go)
        assert out.dtype == dt and xg.grad.dtype == dt and wg.grad.dtype == F32 and sg.grad.dtype == F32
        direct = torch.empty_like(x)
        abi.forward(_view(_flat_view(x, T)), abi.pack_interlace(w, s), 0, 1, out=_view(_flat_view(direct, T)), **KW)
        assert _same_bits(out.detach(), direct)
    with pytest.raises(RuntimeError, match="same type"):
        OPS.temporal_interlace_cl(x.float(), w.double(), s.double(), T, 0, True)


def test_the_node_saves_nothing_of_the_outputs_size():
    shape, T = (6, 8, 4, 5), 3
    N, C = 2, 8
    x = torch.randn(shape, device="cuda").contiguous(memory_format=torch.channels_last)      # (no grad: the caller's tensor, not a copy)
    w, s = torch.zeros(N, C, device="cuda", requires_grad=True), torch.ones(N, T, C, device="cuda", requires_grad=True)
    seen = []

    def pack(t):
        seen.append((tuple(t.shape), t.data_ptr(), t.stride()))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = temporal_interlace_func(x, w, s, T, 0, True, memory_format=KEEP)
    assert out.requires_grad and out.stride() == x.stride()
    assert [sh for sh, _, _ in seen] == [shape, (N, C), (N, T, C)]
    assert seen[0][1] == x.data_ptr() and seen[0][2] == x.stride()      # the one tensor of the output's size is the input as it lies


def test_the_layer_runs_one_fused_call_and_returns_channels_last():
    torch.manual_seed(8)
    N, T, C = 2, 8, 64
    layer = torchshifts.TemporalInterlace(T, C, shift_div=2, memory_format=KEEP).cuda()
    plain = torchshifts.TemporalInterlace(T, C, shift_div=2).cuda()
    plain.load_state_dict(layer.state_dict())
    x = torch.randn(N * T, C, 14, 14, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = layer(x)
    assert abi.last_kernel() == FWD and abi.last_path() == abi.PATH_CL and out.stride() == x.stride()
    assert torch.equal(out.detach(), plain(x.detach())) and abi.last_kernel() == "tinterlace_forward"
    assert torch.equal(out.detach()[:, C // 2:], x.detach()[:, C // 2:])
    out.square().mean().backward()
    assert x.grad.stride() == x.stride()
    for p in layer.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert layer.offset_net.fc2.bias.grad.abs().sum() > 0 and layer.weight_net.conv.weight.grad.abs().sum() > 0
