"""Temporal interlacing on the GPU: SHIFTND_SHIFT_DIM0 | SHIFTND_INTERLACE through the C ABI (csrc/shiftnd_interlace.hip) and through
torch.ops.torchshifts_interlace.  Buffers and views are those of tests/test_tshift_gpu.py -- (N, T, C, M) buffers seen as [N, C, T, M]
problems -- under ONE packed table: the [N, C] offsets followed by the [N, T, C] scales.

The reference is the project's fp64 / fp32 1-D oracle evaluation per clip (tests/test_tshift_gpu.py::_reference's calls) times the
scale: out = oracle_forward(x) * s, grad_x = oracle_backward(s * grad_out), grad_offsets that backward's table gradient in fp64, and
grad_scales[n, t, c] = sum over the plane of grad_out * y in fp64 numpy, y the fp64 forward.

Cases: those of tests/test_per_clip_gpu.py -- whole-piece, ragged, degenerate, and its two chunked ones, the only shapes with several
workgroups per (n, c) line, where the per-step records are indexed across chunks -- and one with 130-element fp32 planes (65 units
of 8 bytes): wave 0 of the workgroup is fully active, wave 1 holds one unit, waves 2 and 3 are idle and must still write their zeros.

Exact data: x and grad_out on eighths, offsets on quarters (rows that differ per clip), scales from {0.5, 1, 2, -1, 0} drawn per
(n, t, c): every product, blend and sum is exact in fp32, so everything is compared bit for bit in all four dtypes.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_interlace_func, temporal_shift_learnable_per_clip_func
from oracle import oracle as O

import redzone as RZ
from exact16_cases import FLOOR16, assert_bits, assert_gw_entries, assert_ulp_close, round16
from test_per_clip_gpu import CHUNKED_CASES, DEGENERATE_CASES, RAGGED_CASES, WHOLE_CASES, _run_per_clip, _table
from test_tshift_gpu import (BWD, BWD_R, FWD, FWD_R, _buffer, _eighths, _frames, _id, _lines, _put, _run, _view, _weights, _whole, _wide)

pytestmark = pytest.mark.gpu

OPS = torch.ops.torchshifts_interlace
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
IFWD, IFWD_R, IBWD, IBWD_R = "tinterlace_forward", "tinterlace_forward_ragged", "tinterlace_backward", "tinterlace_backward_ragged"

WAVES_CASE = ((2, 3, 4, 130), F32, 0)   # 520-byte planes, 65 units of 8 bytes: active, partly active and idle waves in one workgroup
CASES = WHOLE_CASES + RAGGED_CASES + DEGENERATE_CASES + CHUNKED_CASES + [WAVES_CASE]
SWEEP = list(itertools.product(range(5), (0, 1)))
SCALES = np.array([0.5, 1.0, 2.0, -1.0, 0.0])


def _exact_scales(rs, N, T, C):
    """[N, T, C] from SCALES, drawn per entry; every clip, every frame of a clip and every channel of a frame differs somewhere from
    its neighbour, so that a kernel that ignores n, t or c in the scale index fails"""
    while True:
        s = SCALES[rs.randint(0, len(SCALES), size=(N, T, C))]
        if all(len(np.unique(np.moveaxis(s, ax, 0).reshape(s.shape[ax], -1), axis=0)) > 1 or s.shape[ax] == 1 for ax in range(3)):
            return s


def _clip_reference(x, go, w, s, pad, active, dt):
    """one clip.  x, go: (1, T, C, M) arrays of dt's values; w: [C]; s: [T, C] (values of the tables' type).  -> out, grad_x (dt's
    values: the oracle's precision, scaled there, narrowed once), grad_offsets [C] and grad_scales [T, C] in fp64"""
    odt = np.float64 if dt == F64 else np.float32
    xl, wl = _lines(x).astype(odt), w.reshape(-1, 1).astype(odt)
    sb = s.astype(odt)[None, :, :, None]
    out = _frames(O.forward(xl, wl, pad, active), x.shape) * sb                          # the scale after the lerp, its own multiply
    gx = _frames(O.backward(_lines(go.astype(odt) * sb), wl, xl, pad, active)[0], x.shape)   # ... and on the gradient before it
    x64, w64, s64 = _lines(x).astype(np.float64), w.reshape(-1, 1).astype(np.float64), s.astype(np.float64)[None, :, :, None]
    goff = O.backward(_lines(go.astype(np.float64) * s64), w64, x64, pad, active)[1].reshape(-1)
    y64 = _frames(O.forward(x64, w64, pad, active), x.shape)
    gsc = (go.astype(np.float64) * y64).reshape(x.shape[1], x.shape[2], -1).sum(-1)
    if dt in (F16, BF16):
        out, gx = round16(out, dt), round16(gx, dt)
    return out, gx, goff, gsc


def _reference(x, go, w, s, pad, active, dt):
    clips = [_clip_reference(x[n:n + 1], go[n:n + 1], w[n], s[n], pad, active, dt) for n in range(x.shape[0])]
    out, gx = np.concatenate([c[0] for c in clips]), np.concatenate([c[1] for c in clips])
    return out, gx, np.stack([c[2] for c in clips]), np.stack([c[3] for c in clips])


@functools.lru_cache(maxsize=None)
def _inputs(ci, kind, pad, active):
    """x, go (N, T, C, M), offsets [N, C], scales [N, T, C] of CASES[ci] -- fp64 arrays holding values of the case's dtype -- and the
    reference.  Computed once, shared, never written to."""
    shape, dt, _ = CASES[ci]
    N, T, C, M = shape
    rs = np.random.RandomState(7000 + 1000 * ci + 10 * pad + active + (500 if kind == "random" else 0))
    if kind == "exact":
        x, go, w, s = _eighths(rs, shape), _eighths(rs, shape), _table(rs, N, C, T, pad), _exact_scales(rs, N, T, C)
    else:
        narrow = (lambda a: torch.from_numpy(a).to(dt).double().numpy())
        x, go = narrow(rs.uniform(-1, 1, size=shape)), narrow(rs.uniform(-1, 1, size=shape))
        w, s = narrow(_table(rs, N, C, T, pad, quarters=False)), narrow(rs.uniform(-2, 2, size=(N, T, C)))
    ref = _reference(x, go, w, s, pad, active, dt)
    for a in (x, go, w, s) + ref:
        a.setflags(write=False)
    return (x, go, w, s) + ref


def _pack(w, s, dt):
    return torch.from_numpy(np.concatenate([np.asarray(w).reshape(-1), np.asarray(s).reshape(-1)])).to(dt).cuda()


def _run_interlace(shape, dt, off, x, go, w, s, pad, active, wdt=None):
    """the interlace forward and backward on (N, T, C, M) buffers -> out, grad_x, grad_offsets [N, C], grad_scales [N, T, C], the names"""
    N, T, C, M = shape
    table = _pack(w, s, wdt or dt)
    xd, gd = _put(x, dt, off), _put(go, dt, off)
    out, gx = _buffer(shape, dt, off, fill=0xA5), _buffer(shape, dt, off, fill=0xA5)
    abi.forward(_view(xd), table, pad, active, out=_view(out), shift_dim0=True, interlace=True)
    kf = abi.last_kernel()
    assert abi.last_path() == abi.PATH_PLANE
    gt = torch.full_like(table, float("nan"))
    abi.backward(_view(gd), table, _view(xd), pad, active, grad_x=_view(gx), grad_w=gt, shift_dim0=True, interlace=True)
    assert abi.last_path() == abi.PATH_PLANE
    goff, gsc = abi.unpack_interlace(gt, N, T, C)
    return out, gx, goff, gsc, kf, abi.last_kernel()


def _names(shape, dt, off):
    return (IFWD, IBWD) if _whole(shape, dt, off) else (IFWD_R, IBWD_R)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_exact_data(ci):
    shape, dt, off = CASES[ci]
    for pad, active in SWEEP:
        what = (_id(CASES[ci]), "pad", pad, "active", active)
        x, go, w, s, want_out, want_gx, goff64, gsc64 = _inputs(ci, "exact", pad, active)
        out, gx, goff, gsc, kf, kb = _run_interlace(shape, dt, off, x, go, w, s, pad, active)
        assert (kf, kb) == _names(shape, dt, off), what + (kf, kb)
        assert_bits(_wide(out), want_out, what + ("out",))
        assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        if dt in (F32, F64):
            assert np.array_equal(_wide(goff).astype(np.float64), goff64), what + ("grad_offsets",)
            assert np.array_equal(_wide(gsc).astype(np.float64), gsc64), what + ("grad_scales",)
        else:
            assert_bits(_wide(goff), round16(goff64.astype(np.float32), dt), what + ("grad_offsets, the fp64 sum rounded once",))
            assert_bits(_wide(gsc), round16(gsc64.astype(np.float32), dt), what + ("grad_scales, the fp64 sum rounded once",))
            # fp32 tables with the 16-bit tensor: the same bits in out and grad_x, both gradients the sums themselves
            out2, gx2, goff2, gsc2, kf2, kb2 = _run_interlace(shape, dt, off, x, go, w, s, pad, active, wdt=F32)
            assert (kf2, kb2) == _names(shape, dt, off) and goff2.dtype == F32 and gsc2.dtype == F32, what
            assert torch.equal(out2, out) and torch.equal(gx2, gx), what + ("mixed out / grad_x",)
            assert np.array_equal(_wide(goff2).astype(np.float64), goff64), what + ("mixed grad_offsets",)
            assert np.array_equal(_wide(gsc2).astype(np.float64), gsc64), what + ("mixed grad_scales",)


def _check_table(got, want64, dt, what):
    """the bounds of tests/test_tshift_gpu.py::test_random_data for grad_w, on one clip's entries"""
    if dt in (F32, F64):
        err = np.abs(got.astype(np.float64) - want64).max() / max(np.abs(want64).max(), 1e-30)
        print(what, "relative error", err)
        assert err < 1e-5, what + (err,)
    else:
        print(what, "largest error", np.abs(got.astype(np.float64) - want64).max(), "of", np.abs(want64).max())
        assert_gw_entries(got, want64, dt, what)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_random_data(ci):
    """fp32 / fp64: out and grad_x bit-equal to the oracle's no-FMA sequence with the scale as a multiply of its own.  16-bit: the
    sparse shift bit for bit (one product, rounded once), the interpolating one within 1 ulp + FLOOR16 -- the fused op rounds once
    from an fp32 evaluation, and |scale| <= 2 leaves the fp32 difference of the two lerp forms (under 2 ulps of 2^-24) inside the
    floor's 8.  Both gradient tables per clip within the grad_w bounds of the family."""
    shape, dt, off = CASES[ci]
    for pad, active in SWEEP:
        what = (_id(CASES[ci]), "pad", pad, "active", active)
        x, go, w, s, want_out, want_gx, goff64, gsc64 = _inputs(ci, "random", pad, active)
        out, gx, goff, gsc, _, _ = _run_interlace(shape, dt, off, x, go, w, s, pad, active)
        if dt in (F32, F64) or not active:
            assert_bits(_wide(out), want_out, what + ("out",))
            assert_bits(_wide(gx), want_gx, what + ("grad_x",))
        else:
            assert_ulp_close(_wide(out), want_out, dt, FLOOR16, what + ("out",))
            assert_ulp_close(_wide(gx), want_gx, dt, FLOOR16, what + ("grad_x",))
        for n in range(shape[0]):
            _check_table(_wide(goff)[n], goff64[n], dt, what + ("grad_offsets", n))
            _check_table(_wide(gsc)[n].reshape(-1), gsc64[n].reshape(-1), dt, what + ("grad_scales", n))


@pytest.mark.parametrize("ci", [CASES.index(c) for c in CHUNKED_CASES + [((2, 8, 64, 196), F16, 0), WAVES_CASE]])
def test_both_gradient_tables_are_deterministic(ci):
    shape, dt, off = CASES[ci]
    for active in (0, 1):
        x, go, w, s = _inputs(ci, "random", 0, active)[:4]
        a = _run_interlace(shape, dt, off, x, go, w, s, 0, active)
        b = _run_interlace(shape, dt, off, x, go, w, s, 0, active)
        for i in (2, 3):
            assert torch.equal(a[i].contiguous().view(torch.uint8), b[i].contiguous().view(torch.uint8)), (shape, active, i)


def test_the_neighbours_keep_their_kernels():
    """the per-clip and the per-channel flagged calls on one case still report tshift_forward / tshift_backward"""
    shape, dt, off = (2, 3, 5, 8), F16, 0
    rs = np.random.RandomState(71)
    x, go = _eighths(rs, shape), _eighths(rs, shape)
    assert _run_per_clip(shape, dt, off, x, go, _table(rs, 2, 5, 3, 0), 0, 1)[3:] == (FWD, BWD)
    assert _run(shape, dt, off, x, go, _weights(rs, 5, 3, 0), 0, 1)[3:] == (FWD, BWD)


# ---- red zones: every tensor, the packed table, the packed gradient and the workspace between painted zones ---------------------------
GUARDED = [((2, 3, 5, 8), F16), ((2, 3, 5, 49), F32), ((2, 2, 3, 4100), F32)]


@pytest.mark.parametrize("shape,dt", GUARDED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt):
    N, T, C, M = shape
    rs = np.random.RandomState(72)
    dev = torch.device("cuda")
    for pad, active in itertools.product((0, 3), (0, 1)):
        what = (shape, str(dt), "pad", pad, "active", active)
        x, go, w, s = _eighths(rs, shape), _eighths(rs, shape), _table(rs, N, C, T, pad), _exact_scales(rs, N, T, C)
        want_out, want_gx, goff64, gsc64 = _reference(x, go, w, s, pad, active, dt)
        as_dt = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt))
        X, OUT, G, GX = (RZ.Guarded(shape, dt, dev) for _ in range(4))
        W, GW = RZ.Guarded((N * C + N * T * C,), dt, dev), RZ.Guarded((N * C + N * T * C,), dt, dev)
        ws_bytes = abi.backward_workspace(_view(X.t), pad, active, shift_dim0=True, interlace=True).numel()
        chunks = -(-M * X.t.element_size() // 8192)
        assert ws_bytes == chunks * N * C * (1 + 4 * T) * 24, what   # both partial sets, sized exactly
        WS = RZ.Guarded((ws_bytes,), torch.uint8, dev)

        def forward():
            abi.forward(_view(X.t), W.t, pad, active, out=_view(OUT.t), shift_dim0=True, interlace=True)
            return abi.last_kernel()

        def backward():
            abi.backward(_view(G.t), W.t, _view(X.t), pad, active, grad_x=_view(GX.t), grad_w=GW.t, workspace=WS.t, shift_dim0=True,
                         interlace=True)
            return abi.last_kernel()

        table = _pack(w, s, dt).cpu()
        names = _names(shape, dt, 0)
        assert RZ.run_guarded(forward, [("x", X, as_dt(x)), ("table", W, table)], [("out", OUT)], [as_dt(want_out)],
                              what + ("forward",)) == names[0]
        packed64 = np.concatenate([goff64.reshape(-1), gsc64.reshape(-1)])
        want_gt = as_dt(packed64) if dt in (F32, F64) else as_dt(packed64.astype(np.float32))
        assert RZ.run_guarded(backward, [("grad_out", G, as_dt(go)), ("x", X, as_dt(x)), ("table", W, table)],
                              [("grad_x", GX), ("grad_table", GW), ("workspace", WS)], [as_dt(want_gx), want_gt, None],
                              what + ("backward",)) == names[1]


# ---- through the op ---------------------------------------------------------------------------------------------------------------------
def _op_inputs(rs, shape, T, pad, groups=None):
    N, C = shape[0] // T, shape[1]
    G = groups or C
    x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float()
    go = torch.from_numpy(rs.uniform(-1, 1, size=shape)).float()
    w = torch.from_numpy(_table(rs, N, G, T, pad, quarters=False)).float()
    s = torch.from_numpy(rs.uniform(-2, 2, size=(N, T, G))).float()
    return x, go, w, s


def _close(got, want, what):
    """a gradient table against another evaluation of the same sums: within 1e-5 of the largest entry (the family's fp32 bar)"""
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
    print(what, "relative error", err)
    assert err <= 1e-5, what + (err,)


OP_SHAPES = (((6, 5, 4, 8), 3), ((6, 5, 7, 7), 3), ((8, 6), 4), ((4, 3, 4100), 2))


def test_the_op_equals_the_c_abi_and_the_composition():
    """fp32 through the op on HIP tensors: the C-ABI call's bits in everything; the composition run on the GPU (the per-clip op, a
    multiply, autograd) bit for bit in out and input.grad, within the bound in both tables"""
    rs = np.random.RandomState(73)
    for (shape, T), pad, active in itertools.product(OP_SHAPES, range(5), (False, True)):
        what = (shape, pad, active)
        N, C = shape[0] // T, shape[1]
        x, go, w, s = _op_inputs(rs, shape, T, pad)
        xg, wg, sg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
        out = temporal_interlace_func(xg, wg, sg, T, pad, active)
        assert abi.last_kernel() in (IFWD, IFWD_R) and abi.last_path() == abi.PATH_PLANE, what
        out.backward(go.cuda())   # (autograd's thread: the kernel name is per thread, the C-ABI comparison below names the kernel)
        assert out.is_contiguous() and wg.grad.shape == w.shape and sg.grad.shape == s.shape and wg.grad.dtype == F32 and sg.grad.dtype == F32
        # the C ABI on the same buffers
        M = int(np.prod(shape[2:]))
        bshape = (N, T, C, M)
        d_out, d_gx, d_goff, d_gsc, _, _ = _run_interlace(bshape, F32, 0, x.view(bshape).numpy(), go.view(bshape).numpy(), w.numpy(),
                                                          s.numpy(), pad, int(active))
        assert torch.equal(out.detach().view(bshape), d_out) and torch.equal(xg.grad.view(bshape), d_gx), what + ("against the C ABI",)
        assert torch.equal(wg.grad, d_goff) and torch.equal(sg.grad, d_gsc), what + ("tables against the C ABI",)
        # the composition on the GPU
        xc, wc, sc = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
        ref = temporal_shift_learnable_per_clip_func(xc, wc, T, pad, active) * sc.reshape((shape[0], C) + (1,) * (len(shape) - 2))
        ref.backward(go.cuda())
        assert torch.equal(out.detach(), ref.detach()), what + ("out against the composition",)
        assert torch.equal(xg.grad, xc.grad), what + ("input.grad against the composition",)
        _close(wg.grad, wc.grad, what + ("offsets.grad",))
        _close(sg.grad, sc.grad, what + ("scales.grad",))


def test_a_channels_last_input_gives_the_contiguous_result():
    rs = np.random.RandomState(74)
    shape, T = (6, 8, 5, 5), 3
    x, go, w, s = _op_inputs(rs, shape, T, 0)
    xc = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xp = x.cuda().requires_grad_(True)
    wc, wp, sc, sp = (t.cuda().requires_grad_(True) for t in (w, w, s, s))
    out, ref = temporal_interlace_func(xc, wc, sc, T, 0, True), temporal_interlace_func(xp, wp, sp, T, 0, True)
    assert out.is_contiguous() and torch.equal(out, ref)
    out.backward(go.cuda().contiguous(memory_format=torch.channels_last))
    ref.backward(go.cuda())
    assert torch.equal(xc.grad, xp.grad) and torch.equal(wc.grad, wp.grad) and torch.equal(sc.grad, sp.grad)


def test_a_group_table():
    rs = np.random.RandomState(75)
    shape, T, G = (6, 8, 7, 7), 3, 4
    N, C = shape[0] // T, shape[1]
    x, go, w, s = _op_inputs(rs, shape, T, 0, groups=G)
    for active in (False, True):
        xa, wa, sa = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
        xb = x.cuda().requires_grad_(True)
        wb = w.cuda().repeat_interleave(C // G, dim=1).requires_grad_(True)
        sb = s.cuda().repeat_interleave(C // G, dim=2).requires_grad_(True)
        out, ref = temporal_interlace_func(xa, wa, sa, T, 0, active), temporal_interlace_func(xb, wb, sb, T, 0, active)
        out.backward(go.cuda())
        ref.backward(go.cuda())
        assert torch.equal(out, ref) and torch.equal(xa.grad, xb.grad)
        assert wa.grad.shape == (N, G) and torch.equal(wa.grad, wb.grad.view(N, G, C // G).sum(2))
        assert sa.grad.shape == (N, T, G) and torch.equal(sa.grad, sb.grad.view(N, T, G, C // G).sum(3))


def test_autocast_gives_fp32_gradients():
    """fp16 activations with fp32 tables, what torch.autocast hands the op: SHIFTND_WEIGHTS_F32, both table gradients fp32"""
    rs = np.random.RandomState(76)
    shape, T = (6, 5, 4, 8), 3
    x, go, w, s = _op_inputs(rs, shape, T, 0)
    for dt in (F16, BF16):
        xg, wg, sg = x.to(dt).cuda().requires_grad_(True), w.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
        with torch.autocast("cuda", dtype=dt):
            out = temporal_interlace_func(xg, wg, sg, T, 0, True)
        out.backward(go.to(dt).cuda())
        assert out.dtype == dt and xg.grad.dtype == dt and wg.grad.dtype == F32 and sg.grad.dtype == F32
        direct = _buffer((2, T, 5, 32), dt, 0, fill=0xA5)
        abi.forward(_view(xg.detach().view(2, T, 5, 32)), abi.pack_interlace(w.cuda(), s.cuda()), 0, 1, out=_view(direct), shift_dim0=True,
                    interlace=True)
        assert torch.equal(out.detach().view(torch.int16).view(-1), direct.view(torch.int16).view(-1))
    with pytest.raises(RuntimeError, match="same type"):
        OPS.temporal_interlace(x.cuda(), w.double().cuda(), s.double().cuda(), T, 0, True)


def test_the_node_saves_nothing_of_the_outputs_size():
    shape, T = (6, 5, 4, 8), 3
    N, C = 2, 5
    x = torch.randn(shape, device="cuda")                       # (no grad: the input is the caller's tensor, not a copy the node makes)
    w, s = torch.zeros(N, C, device="cuda", requires_grad=True), torch.ones(N, T, C, device="cuda", requires_grad=True)
    seen = []

    def pack(t):
        seen.append((tuple(t.shape), t.data_ptr()))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = temporal_interlace_func(x, w, s, T, 0, True)
    assert out.requires_grad
    assert [sh for sh, _ in seen] == [shape, (N, C), (N, T, C)]
    assert seen[0][1] == x.data_ptr()                           # the one tensor of the output's size is the input itself


def test_the_layer_runs_one_fused_call_and_trains():
    torch.manual_seed(6)
    N, T, C = 2, 8, 64
    layer = torchshifts.TemporalInterlace(T, C, shift_div=2).cuda()
    x = torch.randn(N * T, C, 14, 14, device="cuda", requires_grad=True)
    ref = torchshifts.TemporalInterlace(T, C, shift_div=2)
    ref.load_state_dict(layer.state_dict())
    out = layer(x)
    assert abi.last_kernel() == IFWD
    out.square().mean().backward()
    # the same layer on the CPU.  The two nets agree to a few fp32 ulps of their outputs, so the offsets (in (-2, 2)) differ by under
    # 1e-6; d out / d offset = scale * (x[B] - x[A]), at most 2 * 10 for this normal data: 2e-5 in out, plus fp32 rounding of out itself
    want = ref(x.detach().cpu())
    assert torch.allclose(out.detach().cpu(), want, rtol=1e-5, atol=1e-4)
    assert torch.equal(out.detach()[:, C // 2:], x.detach()[:, C // 2:])
    for p in layer.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert layer.offset_net.fc2.bias.grad.abs().sum() > 0 and layer.weight_net.conv.weight.grad.abs().sum() > 0
