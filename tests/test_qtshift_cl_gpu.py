"""Channels-last quantized interpolating temporal shift on the GPU: shiftnd_forward_quantized under
SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES with an fp32 table (csrc/shiftnd_frames_quant.hip, one kernel: frames_forward_quantized) through
the C ABI on (N, T, M, C) buffers viewed as [N, C, T, M], and through torch.ops.torchshifts_quantized_learnable_cl and
memory_format=torch.preserve_format of torchshifts.quantized.LearnableTemporalShift on HIP tensors.

The reference is tests/test_qtshift_cpu.py's `definition` -- the float CPU op on (int_repr - zp) in fp32 / fp64, rint, + zp, clamp
-- and every comparison is bit for bit.

Paths.  The kernel was built with K = SLOTS = 6.  Per piece (E consecutive channels: 16 one-byte or 4 four-byte elements in a
16-byte piece) and frame t it takes one of three paths, which the GPU cannot report; `piece_paths` below restates the rule in
Python and runs on the CPU on the same tables, and the tables are what reach each path (T = 9):
  uniform_table   floor(w) constant over each piece, differing fractions: every piece, every t, every padding is `uniform`;
  few_table       floor(w) in {-1, 0} alternating inside every piece: the frames t, t + 1, t + 2 (or the fill) -- 3 slots, `few`
                  (`uniform` only where the padding folds them onto one frame, e.g. the last frame under border padding);
  many_table      periodic padding, shifts 0 .. T-1 inside one piece: 8 or 9 distinct frames, more than K: `many`;
  zero_fraction_table   whole shifts and fractions mixed inside every piece: `few`, the whole shifts asking for one slot each;
  tables(C, T)    the ladder of tests/test_qtshift_cpu.py, whatever path its pieces take (mixed pieces, `few` or `many`, under every padding).

Launch plan.  THREADS = 256 threads, P pieces a row, rps = max(1, 256 // P) rows a step, ROWS_IN_FLIGHT = 4 steps a batch, a frame
cut into workgroups while the grid is short of WANT_WORKGROUPS = 6144: `plan` restates the host's arithmetic, and the long-frame
case derives its M from it.
"""
import ctypes

import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.quantized.functional import temporal_shift_learnable_quantized

import redzone as RZ
from test_qtshift_cpu import definition, tables

pytestmark = pytest.mark.gpu

OP = torch.ops.torchshifts_quantized_learnable_cl.temporal_shift_learnable_quantized_cl
PLAIN = torch.ops.torchshifts_quantized_learnable.temporal_shift_learnable_quantized
KERNEL = "frames_forward_quantized"
U8, I8, I32 = torch.uint8, torch.int8, torch.int32
QOF = {U8: torch.quint8, I8: torch.qint8, I32: torch.qint32}
ZP = {U8: 3, I8: -7, I32: 11}
NP = {U8: np.uint8, I8: np.int8, I32: np.int32}
ES = {U8: 1, I8: 1, I32: 4}
RANGE = {U8: (0, 256), I8: (-128, 128), I32: (-2 ** 30, 2 ** 30 + 1)}
SLOTS, THREADS, ROWS_IN_FLIGHT, WANT_WORKGROUPS = 6, 256, 4, 6144   # the constants of csrc/shiftnd_frames_quant.hip


# ---- the path rule and the launch plan, restated ------------------------------------------------------------------------------------
def pad_index(i, n, pad):
    if pad == 1:
        return min(max(i, 0), n - 1)
    if pad == 2:
        return i % n
    if pad == 3:
        m = i % (2 * (n - 1))
        return m if m < n else 2 * (n - 1) - m
    if pad == 4:
        m = i % (2 * n)
        return m if m < n else 2 * n - 1 - m
    return i if 0 <= i < n else -1


def piece_paths(w, T, pad, E):
    """{(piece, t): 'uniform' | 'few' | 'many'} for a [C] table cut into pieces of E elements"""
    w = np.asarray(w, np.float32)
    floor = np.floor(w).astype(np.int64)
    whole = w == np.floor(w)
    out = {}
    for k in range(len(w) // E):
        for t in range(T):
            src = [((0, 0) if T == 1 else (pad_index(t - int(floor[e]), T, pad), pad_index(t + 1 - int(floor[e]), T, pad)))
                   for e in range(k * E, (k + 1) * E)]
            if all(s == src[0] for s in src):
                out[k, t] = "uniform"
                continue
            slots = set()
            for e, (s0, s1) in enumerate(src):
                slots.add(s0)
                slots.add(s0 if whole[k * E + e] else s1)   # (a fraction of exactly 0 asks for the first frame alone)
            out[k, t] = "few" if len(slots) <= SLOTS else "many"
    return out


def plan(N, T, M, P):
    """(rows a step, rows a batch, workgroups a frame, rows of a workgroup): the host's plan for P pieces a row"""
    rps = max(1, THREADS // P)
    batch = rps * ROWS_IN_FLIGHT
    most, wanted = -(-M // batch), -(-WANT_WORKGROUPS // (N * T))
    chunks = min(most, wanted)
    rows = -(-(-(-M // chunks)) // batch) * batch
    return rps, batch, -(-M // rows), rows


def uniform_table(C, E):
    base = np.repeat(np.array([1.0, -2.0, 0.0, 3.0], np.float32)[np.arange(C // E) % 4], E)
    return torch.from_numpy(base + ((np.arange(C) % E) / np.float32(E + 1)).astype(np.float32))


def few_table(C, E):
    return torch.from_numpy(np.where(np.arange(C) % 2 == 0, -1.0, 0.0).astype(np.float32) +
                            ((1 + np.arange(C) % 7) / np.float32(8)).astype(np.float32))


def many_table(C, T):
    return torch.from_numpy(((2 * np.arange(C)) % T + 0.5).astype(np.float32))


def zero_fraction_table(C, E):
    w = few_table(C, E)
    w[::3] = torch.round(w[::3])
    return w


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _view(t):
    """(N, T, M, C) buffer -> the [N, C, T, M] problem the library sees: strides {T*M*C, 1, M*C, C}"""
    return t.permute(0, 3, 1, 2)


def _buffer(shape, dt, off_bytes, fill=None):
    """a dense device tensor of `shape` whose base is `off_bytes` past an aligned allocation"""
    es = torch.empty(0, dtype=dt).element_size()
    flat = torch.empty(int(np.prod(shape)) * es + off_bytes, dtype=torch.uint8, device="cuda")
    if fill is not None:
        flat.fill_(fill)
    t = flat[off_bytes:].view(dt).view(shape)
    assert t.data_ptr() % 16 == off_bytes % 16
    return t


def _data(rs, shape, dt):
    lo, hi = RANGE[dt]
    return rs.randint(lo, hi, size=shape, dtype=np.int64).astype(NP[dt])


def _want(x_np, dt, w, T, pad):
    """the definition on the CPU, in the buffer's (N, T, M, C) order"""
    N, _, M, C = x_np.shape
    q = torch._make_per_tensor_quantized_tensor(torch.from_numpy(np.ascontiguousarray(x_np.transpose(0, 1, 3, 2))).reshape(N * T, C, M),
                                                0.05, ZP[dt])
    return definition(q, w, T, pad).reshape(N, T, C, M).permute(0, 1, 3, 2).contiguous()


def _call(x, w, dt, pad, out, **kw):
    kw.setdefault("active", True)
    kw.setdefault("shift_dim0", True)
    kw.setdefault("frames", True)
    return abi.forward_quantized(_view(x), w, kw.pop("wzp", 0), ZP[dt], pad, out=None if out is None else _view(out), **kw)


def _check(shape, dt, off, pads, ws, seed, kernel=None):
    N, T, M, C = shape
    rs = np.random.RandomState(seed)
    x = _buffer(shape, dt, off)
    for pad in pads:
        x_np = _data(rs, shape, dt)
        x.copy_(torch.from_numpy(x_np))
        for w in ws:
            out = _buffer(shape, dt, off, fill=0xA5)
            _call(x, w.cuda(), dt, pad, out)
            assert abi.last_kernel().startswith(KERNEL) and abi.last_path() == abi.PATH_CL, (shape, abi.last_kernel())
            if kernel is not None:
                assert abi.last_kernel() == kernel, (shape, abi.last_kernel())
            assert torch.equal(out.cpu(), _want(x_np, dt, w, T, pad)), (shape, str(dt), off, "pad", pad, w.tolist())


# (C, dtype, base offset in bytes, the piece in bytes): N = 2, T = 3, M = 5
WIDTHS = [(16, U8, 0, 16), (32, U8, 0, 16), (8, U8, 0, 8), (4, U8, 0, 4), (2, U8, 0, 2), (5, I8, 0, 1), (4, I32, 0, 16), (2, I32, 0, 8),
          (3, I32, 0, 4), (16, U8, 1, 1)]


@pytest.mark.parametrize("case", WIDTHS, ids=lambda c: "C%d-%s-off%d-piece%d" % (c[0], str(c[1]).split(".")[-1], c[2], c[3]))
def test_piece_widths(case):
    C, dt, off, piece = case
    _check((2, 3, 5, C), dt, off, range(5), tables(C, 3), 91, KERNEL if piece == 16 else KERNEL + "_ragged")


PATH_TABLES = ["uniform", "few", "many", "ladder", "zero_fraction"]


def _path_tables(kind, C, E, T):
    return {"uniform": lambda: [uniform_table(C, E)], "few": lambda: [few_table(C, E)], "many": lambda: [many_table(C, T)],
            "ladder": lambda: tables(C, T), "zero_fraction": lambda: [zero_fraction_table(C, E)]}[kind]()


@pytest.mark.parametrize("kind", PATH_TABLES)
@pytest.mark.parametrize("C,dt", [(32, U8), (8, I32)], ids=["C32-uint8", "C8-int32"])
def test_paths(C, dt, kind):
    T, E = 9, 16 // ES[dt]
    ws = _path_tables(kind, C, E, T)
    # how the tables map to the paths for K = 6 (the rule restated on the CPU)
    seen = {pad: set().union(*(set(piece_paths(w, T, pad, E).values()) for w in ws)) for pad in range(5)}
    if kind == "uniform":
        assert all(seen[pad] == {"uniform"} for pad in range(5)), seen
    elif kind in ("few", "zero_fraction"):
        assert all("few" in seen[pad] and "many" not in seen[pad] for pad in range(5)), seen
        if kind == "few":   # floor(w) varies inside EVERY piece
            assert all(len(set(np.floor(ws[0].numpy())[k * E:(k + 1) * E])) == 2 for k in range(C // E))
        else:               # some fractions of a mixed piece are exactly 0
            whole = (ws[0] == torch.floor(ws[0])).view(-1, E)
            assert bool((whole.any(1) & ~whole.all(1)).all())
    elif kind == "many":
        assert "many" in seen[2] and set(piece_paths(ws[0], T, 2, E).values()) == {"many"}, seen
    else:
        assert all(seen[pad] & {"few", "many"} for pad in range(5)), seen   # (far shifts side by side: mixed pieces under every padding)
    _check((2, T, 5, C), dt, 0, range(5), ws, 92, KERNEL)


def test_three_pieces_a_row_leave_the_tail_lanes_idle():
    assert THREADS % 3 != 0
    _check((2, 3, 5, 48), U8, 0, range(5), tables(48, 3), 93, KERNEL)


def test_more_pieces_a_row_than_threads():
    C = 16 * 257
    ws = [torch.from_numpy(np.random.RandomState(94).uniform(-2.5, 2.5, size=C).astype(np.float32)), uniform_table(C, 16)]
    _check((1, 2, 2, C), U8, 0, (0, 3), ws, 94, KERNEL)


def test_several_steps_on_every_path():
    # 16-byte pieces: P = 128 pieces a row, 2 rows a step, 8 rows a batch; M = 11 is a workgroup of a whole batch and one of 3 rows,
    # so the few-frames and the many-frames path (one step at a time) loop, and the uniform path ends on a partial batch
    N, T, M, C = 1, 6, 11, 16 * 128
    rps, batch, chunks, rows = plan(N, T, M, C // 16)
    assert (rps, batch, chunks, rows) == (2, 8, 2, 8)
    wide = torch.from_numpy(np.random.RandomState(95).uniform(-6, 6, size=C).astype(np.float32))
    assert "many" in set(piece_paths(wide, T, 0, 16).values()) and set(piece_paths(few_table(C, 16), T, 0, 16).values()) == {"few"}
    _check((N, T, M, C), U8, 0, (0, 2, 3), [uniform_table(C, 16), few_table(C, 16), wide], 95, KERNEL)


def test_a_long_frame_takes_several_batches_and_several_workgroups():
    # one-byte pieces keep the tensor small: I8, C = 5 -> P = 5 pieces a row.  Enough frames that a frame is cut into 2 workgroups
    # only, and M three rows past four batches: a workgroup of three batches and one of a whole batch and a partial one
    N, T, C = 384, 8, 5
    rps, batch, _, _ = plan(N, T, 1, C)
    M = 4 * batch + 3
    _, _, chunks, rows = plan(N, T, M, C)
    assert chunks > 1 and rows > batch and (M - (chunks - 1) * rows) % batch not in (0,) and M - (chunks - 1) * rows > batch
    assert (M % (rps * ROWS_IN_FLIGHT), chunks, rows) == (3, 2, 3 * batch)
    ws = [torch.tensor([0.25, 1.5, -0.75, 3.0, -2.5]), uniform_table(5, 1) + 0.0]
    _check((N, T, M, C), I8, 0, (0,), ws, 95, KERNEL + "_ragged")


def test_one_frame_a_clip():
    for C, dt in ((32, U8), (5, I8), (4, I32)):
        _check((3, 1, 5, C), dt, 0, range(5), tables(C, 1), 96)


# ---- red zones ------------------------------------------------------------------------------------------------------
RED = [((2, 3, 5, 16), U8, 0, "ladder"), ((2, 3, 5, 5), I8, 0, "ladder"), ((2, 3, 5, 16), U8, 1, "ladder"), ((2, 3, 5, 4), I32, 0, "ladder"),
       ((2, 9, 5, 32), U8, 0, "uniform"), ((2, 9, 5, 32), U8, 0, "few"), ((2, 9, 5, 32), U8, 0, "many")]


@pytest.mark.parametrize("shape,dt,off,kind", RED, ids=lambda v: str(v).split(".")[-1].replace(" ", ""))
def test_red_zones(shape, dt, off, kind):
    N, T, M, C = shape
    rs = np.random.RandomState(97)
    dev = torch.device("cuda")
    w = tables(C, T)[1] if kind == "ladder" else _path_tables(kind, C, 16 // ES[dt], T)[0]
    for pad in ((2,) if kind == "many" else (0, 3)):
        x_np = _data(rs, shape, dt)
        X, OUT = (RZ.Guarded(shape, dt, dev, offset_bytes=off) for _ in range(2))
        W = RZ.Guarded((C,), torch.float32, dev)

        def forward():
            _call(X.t, W.t, dt, pad, OUT.t)
            return abi.last_kernel()

        what = (shape, str(dt), "pad", pad, "offset", off, kind)
        assert RZ.run_guarded(forward, [("x", X, torch.from_numpy(x_np)), ("w", W, w)], [("out", OUT)], [_want(x_np, dt, w, T, pad)],
                              what).startswith(KERNEL)


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_output_untouched():
    shape = (2, 3, 5, 16)
    N, T, M, C = shape
    rs = np.random.RandomState(98)
    x_np = _data(rs, shape, U8)
    x = torch.from_numpy(x_np).cuda()
    w = tables(C, T)[1].cuda()

    def refused(what, call, out, status="invalid argument"):
        with pytest.raises(RuntimeError, match=status):
            call()
        torch.cuda.synchronize()
        assert bool((out.contiguous().view(-1).view(U8) == 0xA5).all()), what

    # segment-major tensors (memory order N, T, C, M seen as [N, C, T, M]) under the pair
    xs = torch.from_numpy(np.ascontiguousarray(x_np.transpose(0, 1, 3, 2))).cuda().transpose(1, 2)
    os_ = _buffer((N, T, C, M), U8, 0, fill=0xA5)
    refused("segment-major views", lambda: abi.forward_quantized(xs, w, 0, ZP[U8], 0, out=os_.transpose(1, 2), shift_dim0=True, frames=True,
                                                                active=True), os_)
    out = _buffer(shape, U8, 0, fill=0xA5)
    refused("segment-major x", lambda: abi.forward_quantized(xs, w, 0, ZP[U8], 0, out=_view(out), shift_dim0=True, frames=True, active=True), out)
    refused("segment-major out", lambda: abi.forward_quantized(_view(x), w, 0, ZP[U8], 0, out=os_.transpose(1, 2), shift_dim0=True, frames=True,
                                                              active=True), os_)
    same = _buffer(shape, U8, 0, fill=0xA5)
    refused("out == x", lambda: _call(same, w, U8, 0, same), same)
    b, new = abi.check_borders([N, C, T, M], [[1, 0], [0, 0]], 2)
    cut = _buffer((N, new[2], new[3], C), U8, 0, fill=0xA5)
    refused("a cut window", lambda: _call(x, w, U8, 0, cut, borders=b), cut)

    def flagged(**bits):
        p = abi.problem(_view(x), 0, True, None, shift_dim0=True, frames=True, **bits)
        abi.check(abi.lib().shiftnd_forward_quantized(ctypes.byref(p), x.data_ptr(), abi.strides5(_view(x)), w.data_ptr(), abi.F32, 0, ZP[U8],
                                                      out.data_ptr(), abi.strides5(_view(out)), abi._stream()), "shiftnd_forward_quantized")

    for bit in ("per_clip", "stream", "clip_frames", "interlace", "interlace_frames"):
        refused("an extra flag bit: " + bit, lambda: flagged(**{bit: True}), out)
    refused("active == 0", lambda: _call(x, w, U8, 0, out, active=False), out, status="unsupported dtype")
    refused("a nonzero w_zero_point", lambda: _call(x, w, U8, 0, out, wzp=1), out)
    # channels-last views under SHIFT_DIM0 alone stay refused
    refused("the flag alone", lambda: _call(x, w, U8, 0, out, frames=False), out)
    _call(x, w, U8, 0, out)   # ... and the call itself is served
    assert abi.last_kernel() == KERNEL and torch.equal(out.cpu(), _want(x_np, U8, w.cpu(), T, 0))


# ---- through the op and the module --------------------------------------------------------------------------------------
def _quantized(rs, shape, dt):
    return torch._make_per_tensor_quantized_tensor(torch.from_numpy(_data(rs, shape, dt)), 0.05, ZP[dt])


def _to_cuda(x, channels_last=False):
    r = x.int_repr().cuda()
    if not channels_last:
        return torch._make_per_tensor_quantized_tensor(r, x.q_scale(), x.q_zero_point())
    # memory order (dim 0, spatial dims, channels): quantize the permuted contiguous tensor, then permute the view back
    order = [0] + list(range(2, r.dim())) + [1]
    back = [0, r.dim() - 1] + list(range(1, r.dim() - 1))
    return torch._make_per_tensor_quantized_tensor(r.permute(order).contiguous(), x.q_scale(), x.q_zero_point()).permute(back)


@pytest.mark.parametrize("dt", [U8, I8, I32], ids=lambda d: str(d).split(".")[-1])
def test_the_op_equals_the_cpu_op(dt):
    rs = np.random.RandomState(99)
    for shape, T in (((6, 16, 5), 3), ((8, 6, 7, 7), 4), ((6, 5, 2, 3, 3), 3)):
        for pad in range(5):
            x = _quantized(rs, shape, dt)
            w = torch.from_numpy(rs.uniform(-T - 1.5, T + 1.5, size=shape[1]).astype(np.float32))
            w[:2] = torch.tensor([0.5, -2.0])
            want = PLAIN(x, w, T, pad, True)
            xd = _to_cuda(x, True)
            assert not xd.is_contiguous() and xd.stride(1) == 1
            for out in (OP(xd, w.cuda().view(-1, 1), T, pad, True),
                        temporal_shift_learnable_quantized(xd, w.cuda(), T, pad, True, memory_format=torch.preserve_format)):
                assert abi.last_kernel().startswith(KERNEL) and abi.last_path() == abi.PATH_CL, (shape, pad, abi.last_kernel())
                assert out.is_cuda and out.dtype == QOF[dt] and out.stride() == xd.stride() and out.shape == x.shape
                assert out.q_scale() == x.q_scale() and out.q_zero_point() == x.q_zero_point()
                assert torch.equal(out.int_repr().cpu(), want.int_repr()), (shape, pad)
            out = OP(_to_cuda(x), w.cuda(), T, pad, True)   # a contiguous input: the existing route
            assert abi.last_kernel() == "tshift_forward_quantized" and out.is_contiguous()
            assert torch.equal(out.int_repr().cpu(), want.int_repr()), (shape, pad)
            sparse = OP(xd, w.cuda(), T, pad, False)        # the sparse shift: temporal_shift_quantized's channels-last route
            assert abi.last_kernel().startswith("frames_forward") and not abi.last_kernel().startswith(KERNEL), abi.last_kernel()
            assert sparse.stride() == xd.stride() and torch.equal(sparse.int_repr().cpu(), PLAIN(x, w, T, pad, False).int_repr()), (shape, pad)


def test_the_module_equals_the_cpu_module():
    rs = np.random.RandomState(100)
    f = torchshifts.LearnableTemporalShift(4, 16, padding="reflect", active_flag=True, sparsity_term=0., memory_format=torch.preserve_format)
    with torch.no_grad():
        f.weight.copy_(torch.from_numpy(rs.uniform(-5, 5, size=(16, 1)).astype(np.float32)))
    m = torchshifts.quantized.LearnableTemporalShift.from_float(f)
    assert m.memory_format == torch.preserve_format
    x = _quantized(rs, (8, 16, 7, 7), U8)
    want = m(x)
    xd = _to_cuda(x, True)
    out = m.cuda()(xd)
    assert abi.last_kernel() == KERNEL and m.weight.is_cuda and out.stride() == xd.stride()
    assert torch.equal(out.int_repr().cpu(), want.int_repr()) and out.q_scale() == want.q_scale() and out.q_zero_point() == want.q_zero_point()


def test_an_empty_tensor_launches_nothing():
    x = torch._make_per_tensor_quantized_tensor(torch.zeros(0, 4, 3, dtype=U8, device="cuda"), 0.1, 3)
    before = abi.last_kernel()
    out = OP(x, torch.zeros(4, device="cuda"), 2, 0, True)
    assert out.shape == x.shape and out.is_quantized and abi.last_kernel() == before
    # ... and at the C ABI under the pair (no frames: N = 0)
    e = torch.zeros(0, 16, 3, 5, dtype=U8, device="cuda").permute(0, 1, 2, 3)
    abi.forward_quantized(e, torch.zeros(16, device="cuda"), 0, 3, 0, out=torch.zeros_like(e), shift_dim0=True, frames=True, active=True)
    assert abi.last_path() == abi.PATH_EMPTY and abi.last_kernel() == before


def test_graph_capture_and_replay():
    rs = np.random.RandomState(101)
    x = _to_cuda(_quantized(rs, (8, 16, 6, 6), U8), True)
    w = torch.linspace(-2.3, 2.3, 16, device="cuda")
    want = OP(x, w, 4, 0, True)
    assert abi.last_kernel() == KERNEL
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        OP(x, w, 4, 0, True)   # (warm-up on the capture stream)
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):   # (a host synchronisation would fail the capture)
            out = OP(x, w, 4, 0, True)
    graph.replay()
    torch.cuda.synchronize()
    assert out.stride() == x.stride() and torch.equal(out.int_repr(), want.int_repr())


# ---- seeded fuzz ----------------------------------------------------------------------------------------------------
def test_seeded_fuzz():
    rs = np.random.RandomState(20261021)
    kinds = set()
    for i in range(150):
        dt = (U8, I8, I32)[rs.randint(3)]
        N, T, C, M = rs.randint(1, 4), rs.randint(1, 10), rs.randint(1, 71), rs.randint(1, 41)
        pad = rs.randint(5)
        off = int(rs.randint(0, 16 // ES[dt])) * ES[dt] if rs.randint(2) else 0
        E = max(1, 16 // ES[dt])
        kind = ("uniform", "few", "many", "ladder")[rs.randint(4)]
        if kind == "ladder":
            w = tables(C, T)[rs.randint(len(tables(C, T)))]
        elif kind == "uniform":
            w = torch.from_numpy(np.repeat(rs.randint(-T - 1, T + 2, size=-(-C // E)), E)[:C].astype(np.float32) +
                                 rs.uniform(0, 0.99, size=C).astype(np.float32))
        elif kind == "few":
            w = torch.from_numpy(rs.uniform(-1, 1, size=C).astype(np.float32))
        else:
            w = torch.from_numpy(rs.uniform(-T, T, size=C).astype(np.float32))
        kinds.add(kind)
        shape = (N, T, M, C)
        x_np = _data(rs, shape, dt)
        x = _buffer(shape, dt, off)
        x.copy_(torch.from_numpy(x_np))
        out = _buffer(shape, dt, off, fill=0xA5)
        _call(x, w.cuda(), dt, pad, out)
        assert abi.last_kernel().startswith(KERNEL) and abi.last_path() == abi.PATH_CL, (i, shape, abi.last_kernel())
        assert torch.equal(out.cpu(), _want(x_np, dt, w, T, pad)), (i, shape, str(dt), "pad", pad, "off", off, kind, w.tolist())
    assert kinds == {"uniform", "few", "many", "ladder"}
