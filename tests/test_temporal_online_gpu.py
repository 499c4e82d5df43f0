"""Online temporal shift on the GPU: SHIFTND_SHIFT_DIM0 | SHIFTND_STREAM (csrc/shiftnd_stream.hip) through the C ABI, and the ops and
modules above it.  A copy op: every comparison is bit for bit, against the oracle's 2-D sparse forward of the [B, C, T, M] view under
(s, 0) (online_cases.reference_frames), five steps each.

Every C-ABI case puts the frame and the state each in the middle of a byte buffer painted with a pattern.  Every guard byte must
keep the paint, and so must every byte of an unshifted channel and of a slot the channel's shift does not reach -- in the state the
initial bytes ARE paint (the cases run against a painted initial state, which the definition allows: the reference for the first
steps is then the painted frame, checked through expected_state and through a second run from a zero state against the oracle).
The shapes are the smallest that reach each branch: 16-, 8-, 4-, 2- and 1-byte pieces in both layouts, more than one workgroup per
stream with a partial last one, B, C or M of 1, one slot and all 15, bases one element off, uniform and mixed channels-last pieces."""
import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_shift_online_func, temporal_shift_online_func_, temporal_shift_online_state
from torchshifts.modules import OnlineTemporalShift
from torchshifts.quantized import OnlineTemporalShift as QOnlineTemporalShift
from torchshifts.quantized.functional import temporal_shift_online_quantized, temporal_shift_online_quantized_

import online_cases as OC
from online_cases import F16, BF16, F32, F64, U8, I8, I32, T

pytestmark = pytest.mark.gpu

WHOLE, RAGGED = "frames_stream", "frames_stream_ragged"
GUARD, PATTERN = 4096, 0x7B
ZP = {U8: 77, I8: -5, I32: 70000}

# (B, C, spatial), dtype, D, base offset in elements, the form
CONTIGUOUS = [
    ((2, 8, (4, 4)), F32, 3, 0, WHOLE),       # 64-byte planes: 16-byte pieces
    ((2, 40, (8, 8)), F32, 3, 0, WHOLE),      # 640 pieces per stream: three workgroups, the last one partial
    ((2, 5, (7, 7)), F16, 3, 0, RAGGED),      # 98-byte planes: 2-byte pieces
    ((3, 6, (14, 14)), BF16, 3, 0, RAGGED),   # 392-byte planes: 8-byte pieces, two workgroups per stream
    ((2, 5, (7, 7)), U8, 3, 0, RAGGED),       # 49-byte planes: 1-byte pieces
    ((2, 3, (2, 2)), F64, 2, 0, WHOLE), ((2, 3, (2, 2)), I32, 3, 0, WHOLE), ((2, 3, (3, 4)), I8, 3, 0, RAGGED),
    ((1, 4, (4, 4)), F32, 3, 0, WHOLE), ((2, 1, (4, 4)), F32, 3, 0, WHOLE), ((2, 8, ()), F32, 3, 0, RAGGED),   # B, C, M of 1
    ((2, 4, (4, 4)), F16, 1, 0, WHOLE), ((2, 4, (2, 2)), F32, 15, 0, WHOLE),                                   # D of 1 and of 15
    ((2, 8, (4, 4)), F32, 3, 1, RAGGED), ((2, 4, (4, 4)), U8, 3, 1, RAGGED), ((2, 3, (2, 4)), F16, 15, 1, RAGGED),   # the base one element off
]
# table: "runs" (constant over runs of 8 channels: uniform pieces) or "random" (mixed pieces)
CHANNELS_LAST = [
    ((2, 16, (3, 3)), F16, 3, 0, WHOLE, "runs"), ((2, 16, (3, 3)), F16, 3, 0, WHOLE, "random"),
    ((2, 12, (3, 3)), F16, 3, 0, RAGGED, "random"),    # 24-byte rows: 8-byte pieces
    ((2, 3, (3, 3)), U8, 3, 0, RAGGED, "random"),      # 3-byte rows: 1-byte pieces
    ((2, 8, (2, 3, 3)), F32, 3, 0, WHOLE, "random"),   # channels_last_3d
    ((2, 8, (5,)), BF16, 3, 0, WHOLE, "random"),       # [B, C, L] with unit channel stride
    ((2, 264, (4, 5)), F16, 2, 0, WHOLE, "runs"),      # 660 pieces per stream: three workgroups, the last one partial
    ((2, 16, (3, 3)), I8, 15, 0, WHOLE, "random"), ((2, 6, (3, 3)), I32, 3, 0, RAGGED, "random"),
    ((2, 16, (3, 3)), F16, 3, 1, RAGGED, "random"), ((2, 16, (3, 3)), U8, 3, 1, RAGGED, "runs"),   # the base one element off
]


def _id(case):
    (B, C, sp), dt, D, off = case[:4]
    return "B%d-C%d-%s-%s-D%d-off%d%s" % (B, C, "x".join(map(str, sp)) or "1", str(dt).split(".")[-1], D, off, "-" + case[5] if len(case) > 5 else "")


class Painted:
    """a dense tensor [lead..., B, C, *spatial] in the middle of a painted byte buffer, contiguous or channels-last in every slot"""

    def __init__(self, lead, geom, dt, off, channels_last):
        B, C, sp = geom
        es = torch.empty(0, dtype=dt).element_size()
        M = int(np.prod(sp)) if sp else 1
        nbytes = int(np.prod(lead, dtype=np.int64)) * B * C * M * es
        self.buffer = torch.full((2 * GUARD + nbytes + 16,), PATTERN, dtype=U8, device="cuda")
        self.lo = GUARD + off * es
        self.hi = self.lo + nbytes
        flat = self.buffer[self.lo:self.hi].view(dt)
        assert flat.data_ptr() % 16 == (off * es) % 16
        n = len(lead)
        if channels_last:
            memory = flat.view(*lead, B, *sp, C)
            self.t = memory.permute(*range(n), n, n + len(sp) + 1, *range(n + 1, n + len(sp) + 1))
        else:
            self.t = flat.view(*lead, B, C, *sp)

    def guards_intact(self):
        return bool((self.buffer[:self.lo] == PATTERN).all()) and bool((self.buffer[self.hi:] == PATTERN).all())


def _paint(dt, shape):
    es = torch.empty(0, dtype=dt).element_size()
    return torch.full(tuple(shape) + (es,), PATTERN, dtype=U8).view(dt).squeeze(-1)


def _table_for(s, dt):
    return s.to(I32 if dt in ZP else (F32 if dt in (F16, BF16) else dt)).cuda()


def _check(geom, dt, D, off, kernel, channels_last, s, rs):
    """five steps from a PAINTED initial state: outputs and state against the definition built on the painted slots (a shifted
    channel of step t < s shows paint), unshifted channels and unreached slots keep the paint; then the frames' stacked outputs of a
    second stream from a zero state against the oracle"""
    B, C, sp = geom
    X, frames = OC.clip(rs, B, C, sp, dt)
    w = _table_for(s, dt)
    for zero_state in (False, True):
        state = Painted((D,), geom, dt, off, channels_last)
        if zero_state:
            state.t.fill_(ZP.get(dt, 0))
            want = OC.reference_frames(X, s, T, 0, ZP.get(dt, 0))
        initial = state.t.cpu().clone()
        for t in range(T):
            frame = Painted((), geom, dt, off, channels_last)
            frame.t.copy_(frames[t])
            abi.online_step(frame.t, state.t, w)
            assert (abi.last_kernel(), abi.last_path()) == (kernel, abi.PATH_CL if channels_last else abi.PATH_PLANE)
            got = frame.t.cpu()
            if zero_state:
                assert OC.same_bits(got, want[t]), (t, s)
            else:
                for c, sc in enumerate(s.tolist()):   # the definition on the painted state
                    src = frames[t][:, c] if sc == 0 else (frames[t - sc][:, c] if t - sc >= 0 else initial[sc - 1 - t][:, c])
                    assert OC.same_bits(got[:, c], src), (t, c, sc)
            assert frame.guards_intact() and state.guards_intact(), t
        assert OC.same_bits(state.t, OC.expected_state(frames, s, initial)), s
        if not zero_state:   # unshifted channels and the slots a shift does not reach: paint
            for c, sc in enumerate(s.tolist()):
                rest = state.t[sc:, :, c].cpu()
                assert OC.same_bits(rest, _paint(dt, rest.shape)), (c, sc)


@pytest.mark.parametrize("case", CONTIGUOUS, ids=_id)
def test_abi_contiguous(case):
    geom, dt, D, off, kernel = case
    rs = np.random.RandomState(len(_id(case)) + geom[1])
    _check(geom, dt, D, off, kernel, False, OC.causal_table(rs, geom[1], D), rs)
    _check(geom, dt, D, off, kernel, False, OC.default_table(geom[1], 4), rs)


@pytest.mark.parametrize("case", CHANNELS_LAST, ids=_id)
def test_abi_channels_last(case):
    geom, dt, D, off, kernel, table = case
    rs = np.random.RandomState(len(_id(case)) + geom[1])
    s = OC.runs_table(geom[1], D) if table == "runs" else OC.causal_table(rs, geom[1], D)
    _check(geom, dt, D, off, kernel, True, s, rs)


def test_entries_outside_the_state_are_clamped():
    rs = np.random.RandomState(2)
    geom, D = (2, 6, (4, 4)), 2
    X, frames = OC.clip(rs, *geom, F32)
    s = torch.tensor([-3, 5, 1, 0, 2, 100])
    clamped = s.clamp(0, D)
    want = OC.reference_frames(X, clamped, T, 0)
    for channels_last in (False, True):
        state = Painted((D,), geom, F32, 0, channels_last)
        state.t.zero_()
        for t in range(T):
            frame = Painted((), geom, F32, 0, channels_last)
            frame.t.copy_(frames[t])
            abi.online_step(frame.t, state.t, s.to(F32).cuda())
            assert OC.same_bits(frame.t, want[t]) and frame.guards_intact() and state.guards_intact()


def test_refused_calls_write_nothing():
    rs = np.random.RandomState(3)
    geom = (2, 4, (2, 2))
    w = torch.ones(4, device="cuda")
    state = Painted((16,), geom, F32, 0, False)   # more slots than the kernel has registers
    frame = Painted((), geom, F32, 0, False)
    x = OC.data(rs, (2, 4, 2, 2), F32)
    frame.t.copy_(x)
    with pytest.raises(RuntimeError, match=r"invalid argument \(-1\)"):
        abi.online_step(frame.t, state.t, w)
    both = Painted((4,), geom, F32, 0, False)     # the frame is a slot of its own state
    with pytest.raises(RuntimeError, match=r"invalid argument \(-1\)"):
        abi.online_step(both.t[1], both.t[:3], w)
    with pytest.raises(RuntimeError, match=r"invalid argument \(-1\)"):
        abi.online_step(frame.t, state.t[:3], w, pad=2)
    torch.cuda.synchronize()
    assert OC.same_bits(frame.t, x) and bool((state.buffer == PATTERN).all()) and bool((both.buffer == PATTERN).all())


# ---- through the ops and the modules -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pad", [0, 1])
def test_float_ops_and_module(pad, channels_last):
    rs = np.random.RandomState(10 + pad + 2 * channels_last)
    for dt, B, C, sp, s in ((F16, 2, 16, (3, 3), OC.default_table(16)), (F32, 2, 5, (2, 3, 3), OC.WRAP), (BF16, 3, 6, (7, 7), None)):
        s = OC.causal_table(rs, C, 4) if s is None else s
        X, frames = OC.clip(rs, B, C, sp, dt)
        want = OC.reference_frames(X, s, T, pad)
        first = OC.layout(frames[0].cuda(), channels_last)
        state = temporal_shift_online_state(first, s.cuda(), pad)
        assert state.stride()[1:] == first.stride() and state.is_cuda
        for t in range(T):
            f = OC.layout(frames[t].cuda(), channels_last)
            strides, versions = f.stride(), (f._version, state._version)
            if t % 2:
                out = temporal_shift_online_func(f, state, s.cuda())
                assert out is not f and OC.same_bits(f, frames[t])
            else:
                out = temporal_shift_online_func_(f, state, s.cuda())
                assert out is f and f._version > versions[0]
            assert out.stride() == strides and state._version > versions[1]
            assert abi.last_kernel() in (WHOLE, RAGGED)
            assert OC.same_bits(out, want[t]), (dt, pad, t)
    m = OnlineTemporalShift(16, padding="border" if pad else "zeros", inplace=True).cuda()
    X, frames = OC.clip(rs, 2, 16, (3, 3), F16)
    want = OC.reference_frames(X, m.shifts.cpu(), T, pad)
    for t in range(T):
        f = OC.layout(frames[t].cuda(), channels_last)
        assert m(f) is f and OC.same_bits(f, want[t])
    assert m._table.dtype == F32 and m.state.is_cuda


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pad", [0, 1])
def test_quantized_ops_and_module(pad, channels_last):
    rs = np.random.RandomState(20 + pad + 2 * channels_last)
    for dt in (U8, I8, I32):
        s = OC.causal_table(rs, 16, 3)
        X, frames = OC.clip(rs, 2, 16, (3, 3), dt)
        want = OC.reference_frames(X, s, T, pad, ZP[dt])
        first = OC.quantized(frames[0].cuda(), ZP[dt], channels_last)
        state = temporal_shift_online_state(first, s.cuda(), pad)
        assert state.is_quantized and state.stride()[1:] == first.stride() and state.q_zero_point() == ZP[dt]
        for t in range(T):
            q = OC.quantized(frames[t].cuda(), ZP[dt], channels_last)
            out = (temporal_shift_online_quantized if t % 2 else temporal_shift_online_quantized_)(q, state, s.cuda())
            assert (out is q) == (t % 2 == 0) and out.stride() == q.stride() and out.q_zero_point() == ZP[dt] and out.q_scale() == 0.05
            assert abi.last_kernel() in (WHOLE, RAGGED)
            assert OC.same_bits(out.int_repr(), want[t]), (dt, pad, t)
    q = QOnlineTemporalShift.from_float(OnlineTemporalShift(16, padding="border" if pad else "zeros")).cuda()
    X, frames = OC.clip(rs, 2, 16, (3, 3), U8)
    want = OC.reference_frames(X, q.shifts.cpu(), T, pad, 77)
    for t in range(T):
        f = OC.quantized(frames[t].cuda(), 77, channels_last)
        out = q(f)
        assert out is not f and OC.same_bits(out.int_repr(), want[t]) and OC.same_bits(f.int_repr(), frames[t])
    assert q._table.dtype == I32


def test_sixteen_slots_and_views_take_the_composite_with_the_same_values():
    rs = np.random.RandomState(30)
    s = torch.tensor([16, 0, 3, 1, 7])
    X, frames = OC.clip(rs, 2, 5, (2, 2), F16, steps=18)
    want = OC.reference_frames(X, s, 18, 0)
    state = temporal_shift_online_state(frames[0].cuda(), s.cuda(), 0)
    assert state.shape[0] == 16
    before = abi.last_kernel()
    for t in range(18):
        assert OC.same_bits(temporal_shift_online_func_(frames[t].cuda(), state, s.cuda()), want[t]), t
    assert abi.last_kernel() == before   # no C-ABI kernel ran
    # a frame that is a slice of a wider tensor: not dense
    X, frames = OC.clip(rs, 2, 9, (3, 3), F32)
    s9 = OC.causal_table(rs, 5, 3)
    want = OC.reference_frames(X[:, 2:7], s9, T, 0)
    state = temporal_shift_online_state(frames[0].cuda()[:, 2:7], s9.cuda(), 0)
    for t in range(T):
        base = frames[t].cuda()
        temporal_shift_online_func_(base[:, 2:7], state, s9.cuda())
        assert OC.same_bits(base[:, 2:7], want[t])
        assert OC.same_bits(base[:, :2], frames[t][:, :2]) and OC.same_bits(base[:, 7:], frames[t][:, 7:])
    with pytest.raises(RuntimeError, match="temporal_shift_online_: a negative shift reads the future"):
        temporal_shift_online_func_(base[:, 2:7], state, -s9.cuda())


@pytest.mark.parametrize("channels_last", [False, True])
def test_no_allocation_inside_a_step(channels_last):
    m = OnlineTemporalShift(64, inplace=True).cuda()
    x = OC.layout(torch.randn(4, 64, 8, 8, device="cuda", dtype=F16), channels_last)
    m(x)   # (the first call makes the state and the table, and loads what a first call loads)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m(x)
    temporal_shift_online_func_(x, m.state, m._table)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base and torch.cuda.max_memory_allocated() == base
    assert abi.last_kernel() == WHOLE


@pytest.mark.parametrize("channels_last", [False, True])
def test_a_captured_step_replayed_five_times(channels_last):
    rs = np.random.RandomState(40)
    X, frames = OC.clip(rs, 2, 16, (4, 4), F16)
    s = OC.runs_table(16, 2)
    want = OC.reference_frames(X, s, T, 0)
    static = OC.layout(torch.zeros(2, 16, 4, 4, dtype=F16, device="cuda"), channels_last)
    m = OnlineTemporalShift(16, shifts=s, inplace=True).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(static)   # warm-up outside the capture: the state and the table exist from here on
    torch.cuda.current_stream().wait_stream(side)
    m.state.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m(static)
    m.state.zero_()   # (capture ran nothing)
    for t in range(T):
        static.copy_(frames[t].cuda())
        graph.replay()
        assert OC.same_bits(static, want[t]), t
