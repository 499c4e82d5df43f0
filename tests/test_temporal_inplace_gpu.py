"""In-place temporal shift on the GPU: out == x under SHIFTND_SHIFT_DIM0 (csrc/shiftnd_inplace.hip) through the C ABI, and the ops and
modules above it.  A copy op: every comparison is bit for bit, against the oracle's 2-D sparse forward of the [N, C, T, M] view under
(s, 0) computed from a clone taken before the call (inplace_cases.reference).

Every C-ABI case runs on a slice out of the middle of a byte buffer painted with a pattern, and every guard byte must keep it.  The
shapes are the smallest that reach each branch: 16-, 8-, 4-, 2- and 1-byte pieces in both layouts, more than one workgroup per clip
with a partial last one, N, C, M or T of 1, all 16 frame slots, bases one element off, uniform and mixed channels-last pieces."""
import numpy as np
import pytest
import torch

import torchshifts
from torchshifts import abi
from torchshifts.functional import temporal_shift_func, temporal_shift_func_
from torchshifts.modules import TemporalShift
from torchshifts.quantized import TemporalShift as QTemporalShift
from torchshifts.quantized.functional import temporal_shift_quantized, temporal_shift_quantized_

import inplace_cases as IC
from inplace_cases import F16, BF16, F32, F64, U8, I8, I32, PADS

pytestmark = pytest.mark.gpu

WHOLE, RAGGED = "frames_inplace", "frames_inplace_ragged"
GUARD, PATTERN = 4096, 0x7B
ZP = {U8: 77, I8: -5, I32: 70000}
GIB = 1 << 30

# (N, T, C, spatial), dtype, base offset in elements, the form
CONTIGUOUS = [
    ((2, 4, 8, (4, 4)), F32, 0, WHOLE),       # 64-byte planes: 16-byte pieces
    ((2, 4, 40, (8, 8)), F32, 0, WHOLE),      # 640 pieces per frame: three workgroups per clip, the last one partial
    ((2, 3, 5, (7, 7)), F16, 0, RAGGED),      # 98-byte planes: 2-byte pieces
    ((3, 8, 6, (14, 14)), BF16, 0, RAGGED),   # 392-byte planes: 8-byte pieces, two workgroups per clip
    ((2, 4, 5, (7, 7)), U8, 0, RAGGED),       # 49-byte planes: 1-byte pieces
    ((2, 2, 3, (2, 2)), F64, 0, WHOLE), ((2, 4, 3, (2, 2)), I32, 0, WHOLE), ((2, 4, 3, (3, 4)), I8, 0, RAGGED),
    ((1, 4, 4, (4, 4)), F32, 0, WHOLE), ((2, 4, 1, (4, 4)), F32, 0, WHOLE), ((2, 4, 8, ()), F32, 0, RAGGED),   # N, C, M of 1
    ((3, 1, 4, (4, 4)), F32, 0, WHOLE), ((2, 2, 4, (4, 4)), F16, 0, WHOLE), ((1, 16, 4, (2, 2)), F32, 0, WHOLE),   # T of 1, 2, 16
    ((2, 4, 8, (4, 4)), F32, 1, RAGGED), ((2, 4, 4, (4, 4)), U8, 1, RAGGED), ((2, 16, 3, (2, 4)), F16, 1, RAGGED),   # the base one element off
]
# table: "runs" (constant over runs of 8 channels: uniform pieces) or "random" (mixed pieces)
CHANNELS_LAST = [
    ((2, 4, 16, (3, 3)), F16, 0, WHOLE, "runs"), ((2, 4, 16, (3, 3)), F16, 0, WHOLE, "random"),
    ((2, 4, 12, (3, 3)), F16, 0, RAGGED, "random"),    # 24-byte rows: 8-byte pieces
    ((2, 4, 3, (3, 3)), U8, 0, RAGGED, "random"),      # 3-byte rows: 1-byte pieces
    ((2, 4, 8, (3, 3)), F32, 0, WHOLE, "random"), ((2, 4, 4, (3, 3)), F64, 0, WHOLE, "random"), ((2, 4, 16, (3, 3)), I8, 0, WHOLE, "random"),
    ((2, 4, 6, (3, 3)), I32, 0, RAGGED, "random"),     # 24-byte rows of dwords
    ((2, 4, 8, (2, 3, 3)), F32, 0, WHOLE, "random"),   # channels_last_3d
    ((2, 4, 8, (5,)), BF16, 0, WHOLE, "random"),       # [N*T, C, L] with unit channel stride
    ((2, 16, 64, (5, 5)), F16, 0, WHOLE, "random"),    # 200 pieces per frame and all 16 slots
    ((3, 8, 264, (4, 5)), F16, 0, WHOLE, "runs"),      # 660 pieces per frame: three workgroups per clip, the last one partial
    ((2, 4, 16, (3, 3)), F16, 1, RAGGED, "random"), ((2, 4, 16, (3, 3)), U8, 1, RAGGED, "runs"),   # the base one element off
]


def _id(case):
    (N, T, C, sp), dt, off = case[:3]
    return "N%d-T%d-C%d-%s-%s-off%d%s" % (N, T, C, "x".join(map(str, sp)) or "1", str(dt).split(".")[-1], off, "-" + case[4] if len(case) > 4 else "")


class Painted:
    """a dense tensor in the middle of a painted byte buffer.  .t: the [N*T, C, *spatial] tensor; .view: the [N, C, T, M] problem"""

    def __init__(self, geom, dt, off, channels_last):
        N, T, C, sp = geom
        M = int(np.prod(sp)) if sp else 1
        es = torch.empty(0, dtype=dt).element_size()
        nbytes = N * T * C * M * es
        self.buffer = torch.full((2 * GUARD + nbytes + 16,), PATTERN, dtype=U8, device="cuda")
        self.lo = GUARD + off * es
        self.hi = self.lo + nbytes
        flat = self.buffer[self.lo:self.hi].view(dt)
        assert flat.data_ptr() % 16 == (off * es) % 16
        if channels_last:
            memory = flat.view(N * T, *sp, C)
            self.t = memory.permute(0, len(sp) + 1, *range(1, len(sp) + 1))
            self.view = flat.view(N, T, M, C).permute(0, 3, 1, 2)
        else:
            self.t = flat.view(N * T, C, *sp)
            self.view = flat.view(N, T, C, M).permute(0, 2, 1, 3)

    def guards_intact(self):
        return bool((self.buffer[:self.lo] == PATTERN).all()) and bool((self.buffer[self.hi:] == PATTERN).all())


def _call(p, s, dt, pad):
    """the in-place C-ABI call on p.view under the integer table s; the table as the ops build it"""
    if dt in ZP:
        abi.forward_quantized(p.view, s.to(I32).cuda(), 0, ZP[dt], pad, out=p.view, shift_dim0=True)
    else:
        abi.forward(p.view, s.to(F32 if dt in (F16, BF16) else dt).cuda(), pad, 0, out=p.view, shift_dim0=True)
    return abi.last_kernel(), abi.last_path()


def _check(geom, dt, off, kernel, channels_last, s, pad, rs):
    N, T, C, sp = geom
    p = Painted(geom, dt, off, channels_last)
    x = IC.data(rs, tuple(p.t.shape), dt)
    p.t.copy_(x)
    want = IC.reference(x, s, T, pad, ZP.get(dt, 0))
    got = _call(p, s, dt, pad)
    assert got == (kernel, abi.PATH_CL if channels_last else abi.PATH_PLANE), got
    assert IC.same_bits(p.t, want), (pad, s)
    assert p.guards_intact(), pad


def _runs_table(C, T):
    s = torch.zeros(C, dtype=torch.int64)
    for k, v in enumerate((-1, 1, T + 1, 0, -2, 2 * T)):
        s[8 * k:8 * (k + 1)] = v
    return s


@pytest.mark.parametrize("case", CONTIGUOUS, ids=_id)
def test_abi_contiguous(case):
    geom, dt, off, kernel = case
    rs = np.random.RandomState(len(_id(case)) + geom[2])
    for pad in PADS:
        _check(geom, dt, off, kernel, False, IC.random_table(rs, geom[2], geom[1]), pad, rs)
    _check(geom, dt, off, kernel, False, IC.published_table(geom[2], 4), 0, rs)


@pytest.mark.parametrize("case", CHANNELS_LAST, ids=_id)
def test_abi_channels_last(case):
    geom, dt, off, kernel, table = case
    rs = np.random.RandomState(len(_id(case)) + geom[2])
    for pad in PADS:
        s = _runs_table(geom[2], geom[1]) if table == "runs" else IC.random_table(rs, geom[2], geom[1])
        _check(geom, dt, off, kernel, True, s, pad, rs)


@pytest.mark.parametrize("channels_last", [False, True])
def test_more_frames_than_slots_is_refused_and_nothing_is_written(channels_last):
    rs = np.random.RandomState(3)
    for dt in (F16, U8):
        p = Painted((2, 17, 8, (2, 2)), dt, 0, channels_last)
        x = IC.data(rs, tuple(p.t.shape), dt)
        p.t.copy_(x)
        with pytest.raises(RuntimeError, match=r"invalid argument \(-1\)"):
            _call(p, IC.random_table(rs, 8, 17), dt, 0)
        torch.cuda.synchronize()
        assert IC.same_bits(p.t, x) and p.guards_intact()


@pytest.mark.parametrize("channels_last", [False, True])
def test_an_all_zero_table_leaves_every_bit(channels_last):
    for dt in (F32, F16, F64):
        p = Painted((2, 8, 16, (4, 4)), dt, 0, channels_last)
        es = torch.empty(0, dtype=dt).element_size()
        x = torch.randint(0, 256, tuple(p.t.shape) + (es,), dtype=U8).view(dt).squeeze(-1).clone()   # random bits: NaN payloads, infinities, denormals
        x.view(-1)[::7] = float("nan")
        x.view(-1)[3::7] = -0.0
        p.t.copy_(x)
        for pad in PADS:
            assert _call(p, torch.zeros(16, dtype=torch.int64), dt, pad)[0] == WHOLE
            assert IC.same_bits(p.t, x) and p.guards_intact(), (dt, pad)
        # ... and so does a whole period under periodic padding
        _call(p, torch.full((16,), 8, dtype=torch.int64), dt, 2)
        assert IC.same_bits(p.t, x), dt


# ---- through the ops and the modules ------------------------------------------------------------------------------------------
def _layout(t, channels_last):
    if not channels_last:
        return t.contiguous()
    return t.contiguous(memory_format=torch.channels_last if t.dim() == 4 else torch.channels_last_3d)


def _quantized(int_repr, zp, channels_last):
    if not channels_last:
        return torch._make_per_tensor_quantized_tensor(int_repr.contiguous(), 0.05, zp)
    order = [0] + list(range(2, int_repr.dim())) + [1]
    back = [0, int_repr.dim() - 1] + list(range(1, int_repr.dim() - 1))
    return torch._make_per_tensor_quantized_tensor(int_repr.permute(order).contiguous(), 0.05, zp).permute(back)


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("T", [8, 17])
def test_float_op_and_module(T, channels_last):
    rs = np.random.RandomState(T + channels_last)
    for dt, shape in ((F16, (2 * T, 16, 3, 3)), (F32, (T, 8, 2, 3, 3)), (BF16, (2 * T, 6, 7, 7))):
        for pad in PADS:
            s = IC.random_table(rs, shape[1], T)
            cpu = IC.data(rs, shape, dt)
            want = IC.reference(cpu, s, T, pad)
            x = _layout(cpu.cuda(), channels_last)
            strides, version, base = x.stride(), x._version, x.data_ptr()
            assert temporal_shift_func_(x, s.cuda(), T, pad) is x
            assert x.stride() == strides and x._version > version and x.data_ptr() == base
            assert IC.same_bits(x, want), (dt, pad)
            if T <= 16:
                assert abi.last_kernel() in (WHOLE, RAGGED)
    m = TemporalShift(T, 16, padding="border", inplace=True).cuda()
    cpu = IC.data(rs, (2 * T, 16, 3, 3), F16)
    x = _layout(cpu.cuda(), channels_last)
    assert m(x) is x and IC.same_bits(x, IC.reference(cpu, m.shifts, T, 1))


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("T", [8, 17])
def test_quantized_op_and_module(T, channels_last):
    rs = np.random.RandomState(10 + T + channels_last)
    for dt in (U8, I8, I32):
        for pad in PADS:
            s = IC.random_table(rs, 16, T)
            cpu = IC.data(rs, (2 * T, 16, 3, 3), dt)
            want = IC.reference(cpu, s, T, pad, ZP[dt])
            x = _quantized(cpu.cuda(), ZP[dt], channels_last)
            strides, version = x.stride(), x._version
            assert temporal_shift_quantized_(x, s.cuda(), T, pad) is x
            assert x.stride() == strides and x._version > version and x.q_zero_point() == ZP[dt] and x.q_scale() == 0.05
            assert IC.same_bits(x.int_repr(), want), (dt, pad)
            if T <= 16:
                assert abi.last_kernel() in (WHOLE, RAGGED)
    q = QTemporalShift.from_float(TemporalShift(T, 16, inplace=True)).cuda()
    cpu = IC.data(rs, (2 * T, 16, 3, 3), U8)
    x = _quantized(cpu.cuda(), 77, channels_last)
    assert q(x) is x and IC.same_bits(x.int_repr(), IC.reference(cpu, q.shifts, T, 0, 77))


def test_a_slice_falls_back_and_is_updated_through_its_base():
    rs = np.random.RandomState(21)
    s = IC.random_table(rs, 4, 4)
    cpu = IC.data(rs, (8, 9, 5, 5), F16)
    base = cpu.cuda()
    piece = base[:, 2:6, 1:4]
    want = IC.reference(cpu[:, 2:6, 1:4], s, 4, 0)
    assert temporal_shift_func_(piece, s.cuda(), 4, 0) is piece
    assert IC.same_bits(base[:, 2:6, 1:4], want)
    outside = torch.ones(cpu.shape, dtype=torch.bool)
    outside[:, 2:6, 1:4] = False
    assert torch.equal(base.cpu()[outside], cpu[outside])
    qcpu = IC.data(rs, (8, 9, 5, 5), U8)
    qbase = torch._make_per_tensor_quantized_tensor(qcpu.cuda(), 0.05, 9)
    temporal_shift_quantized_(qbase[:, 2:6], s.cuda(), 4, 0)
    assert IC.same_bits(qbase.int_repr()[:, 2:6], IC.reference(qcpu[:, 2:6], s, 4, 0, 9))
    assert torch.equal(qbase.int_repr().cpu()[:, :2], qcpu[:, :2]) and torch.equal(qbase.int_repr().cpu()[:, 6:], qcpu[:, 6:])


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("T", [8, 17])
def test_gradients_match_the_out_of_place_op(T, channels_last):
    rs = np.random.RandomState(30 + T)
    keep = torch.preserve_format if channels_last else torch.contiguous_format
    for dt in (F32, F16):
        for pad in PADS:
            s = IC.random_table(rs, 16, T).cuda()
            a = _layout(IC.data(rs, (2 * T, 16, 3, 3), dt).cuda(), channels_last).requires_grad_()
            b = a.detach().clone(memory_format=torch.preserve_format).requires_grad_()
            g = _layout(IC.data(rs, (2 * T, 16, 3, 3), dt).cuda(), channels_last)
            out = temporal_shift_func_(a * 1, s, T, pad)
            out.backward(g)
            ref = temporal_shift_func(b * 1, s, T, pad, keep)
            ref.backward(g)
            assert IC.same_bits(out, ref) and IC.same_bits(a.grad, b.grad), (dt, pad)
            assert a.grad.stride() == b.grad.stride()
            assert a.grad.is_contiguous(memory_format=torch.channels_last) == channels_last


def test_no_allocation_of_the_inputs_size():
    T, shape = 8, (64, 64, 32, 32)   # 8 MiB of fp16
    s = IC.published_table(64).cuda()
    for channels_last in (False, True):
        x = _layout(torch.randn(shape, device="cuda", dtype=F16), channels_last)
        assert x.numel() * x.element_size() == 8 << 20
        temporal_shift_func_(x, s, T, 0)   # (the first call loads what a first call loads)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        temporal_shift_func_(x, s, T, 0)
        torch.cuda.synchronize()
        inplace_rise = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = temporal_shift_func(x, s, T, 0, torch.preserve_format)
        torch.cuda.synchronize()
        plain_rise = torch.cuda.max_memory_allocated() - base
        del out
        assert plain_rise >= 8 << 20, plain_rise   # the probe sees an allocation of the input's size
        assert inplace_rise < 1 << 20, inplace_rise


# ---- past the 32-bit limits --------------------------------------------------------------------------------------------------------
def _need(gib, what):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GIB:
        pytest.skip("%s needs %.1f GiB of device memory, %.1f GiB are free" % (what, gib, free / GIB))


def _idiom(v, fold, fill):
    """the published module's slicing on a [N, T, C, ...] (or [N, T, ..., C] with channel_dim -1) clone"""
    out = torch.full_like(v, fill)
    out[:, :-1, :fold] = v[:, 1:, :fold]
    out[:, 1:, fold:2 * fold] = v[:, :-1, fold:2 * fold]
    out[:, :, 2 * fold:] = v[:, :, 2 * fold:]
    return out


def test_contiguous_bytes_past_4_gib():
    _need(13.5, "the uint8 tensor of 2^32 + 2^20 bytes, its clone and the idiom's result")
    T, C, H, W = 8, 64, 4097, 2048
    x = torch.empty(T, C, H, W, dtype=U8, device="cuda").random_(0, 256)
    assert x.numel() == 2 ** 32 + 2 ** 20
    want = _idiom(x.clone().view(1, T, C, H, W), C // 8, 77).view(T, C, H, W)
    view = x.view(1, T, C, H * W).permute(0, 2, 1, 3)
    abi.forward_quantized(view, IC.published_table(C).to(I32).cuda(), 0, 77, 0, out=view, shift_dim0=True)
    assert abi.last_kernel() == WHOLE and abi.last_path() == abi.PATH_PLANE
    assert torch.equal(x, want)
    del x, want, view
    torch.cuda.empty_cache()


def test_channels_last_fp16_past_2_31_elements():
    _need(13.5, "the fp16 tensor past 2^31 elements, its clone and the idiom's result")
    T, C, H, W = 8, 64, 65537, 64
    memory = torch.empty(T, H, W, C, dtype=torch.int16, device="cuda").random_(0, 30000).view(F16)   # finite values (the comparison is torch.equal)
    assert memory.numel() == 2 ** 31 + 2 ** 15
    want = _idiom(memory.clone().view(1, T, H * W, C).permute(0, 1, 3, 2), C // 8, 0.0)   # [N, T, C, M] view of the clone
    x = memory.permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=torch.channels_last)
    assert temporal_shift_func_(x, IC.published_table(C).cuda(), T, 0) is x
    assert abi.last_kernel() == WHOLE and abi.last_path() == abi.PATH_CL
    assert torch.equal(memory.view(1, T, H * W, C).permute(0, 1, 3, 2), want)
    del memory, want, x
    torch.cuda.empty_cache()
