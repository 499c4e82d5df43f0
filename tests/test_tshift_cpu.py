"""The learnable temporal shift on CPU tensors: torch.ops.torchshifts.temporal_shift_learnable, temporal_shift_learnable_func, the
LearnableTemporalShift module and TemporalShift.from_shift against the definition

    shift1d_func(x.view(N, T, C, M).permute(0, 3, 2, 1).reshape(N*M, C, T), w.view(C, 1), pad, active)
        .view(N, M, C, T).permute(0, 3, 2, 1).reshape(x.shape)

and autograd's gradients of that expression.  The CPU key IS that expression on the CPU 1-D ops, so every comparison is bit for bit.
"""
import numpy as np
import pytest
import torch

import torchshifts
from torchshifts.functional import shift1d_func, temporal_shift_learnable_func

OPS = torch.ops.torchshifts
SHAPES = [((6, 5, 4, 8), 3), ((8, 6), 4)]


def definition(x, w, T, pad, active):
    NT, C = x.shape[:2]
    N, M = NT // T, x.numel() // (NT * C)
    lines = x.view(N, T, C, M).permute(0, 3, 2, 1).reshape(N * M, C, T)
    return shift1d_func(lines, w.view(C, 1), pad, active).view(N, M, C, T).permute(0, 3, 2, 1).reshape(x.shape)


def weights(rs, C, T, dt):
    """0, an exact integer, T + 1, -(T + 1), 0.5, -0.25, then quarters in [-(T + 1), T + 1]"""
    w = rs.randint(-4 * (T + 1), 4 * (T + 1) + 1, size=C) / 4.0
    special = [0.0, 2.0, T + 1.0, -(T + 1.0), 0.5, -0.25]
    w[:min(C, 6)] = special[:C]
    return torch.from_numpy(w).to(dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("shape,T", SHAPES, ids=["6x5x4x8", "8x6"])
def test_the_op_equals_the_definition(shape, T, dt):
    rs = np.random.RandomState(21)
    for pad in range(5):
        for active in (False, True):
            for wshape in ((-1,), (-1, 1)):
                x = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt)
                go = torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dt)
                w = (weights(rs, shape[1], T, dt) + (0.125 if active else 0.0)).reshape(wshape)
                xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
                out = temporal_shift_learnable_func(xa, wa, T, pad, active)
                out.backward(go)
                xb, wb = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
                ref = definition(xb, wb, T, pad, active)
                ref.backward(go)
                what = (shape, T, pad, active, wshape)
                assert out.shape == x.shape and torch.equal(out, ref), what
                assert torch.equal(xa.grad, xb.grad), what
                assert wa.grad.shape == w.shape and torch.equal(wa.grad, wb.grad), what
                assert torch.equal(OPS.temporal_shift_learnable(x, w, T, pad, active), out.detach()), what


def test_the_sparse_mode_is_the_fixed_temporal_shift_under_rint():
    rs = np.random.RandomState(22)
    x = torch.from_numpy(rs.uniform(-1, 1, size=(6, 5, 7, 7))).float()
    w = weights(rs, 5, 3, torch.float32)
    for pad in range(5):
        assert torch.equal(OPS.temporal_shift_learnable(x, w, 3, pad, False), OPS.temporal_shift(x, torch.round(w), 3, pad)), pad


def test_gradient_check_of_the_active_form():
    """Fractions away from 0 and 1: the interpolation is smooth there.

    What a gradient check can hold the op to follows from the definition, whose gradients are shift1d's, i.e. the reference's
    backward rule.  weights.grad is calculus under every padding: sum of grad_out * (x[t - iw + 1] - x[t - iw]).  The active
    input gradient is NOT the adjoint of the forward: the reference blends grad_out at t - iw and t - iw + 1 with (1 - d, d) where
    the adjoint would take t + iw and t + iw - 1 (kernels/shifts_kernels.h:272-276, restated in oracle/shift_oracle.c), and the op
    returns that rule bit for bit (test_the_op_equals_the_definition).  With T = 2 the two index pairs are congruent modulo 2, the
    period of the periodic and of the reflect map on two frames, so there the rule IS the adjoint and the full check (input and
    weights) applies; under zeros / border / symmetric it differs by up to d * |grad_out| and only the weights are checked."""
    rs = np.random.RandomState(23)
    x = torch.from_numpy(rs.uniform(-1, 1, size=(4, 3, 2, 2))).double().requires_grad_(True)
    w = torch.tensor([0.3, -0.6, 1.45], dtype=torch.float64, requires_grad=True)
    for pad in (2, 3):
        assert torch.autograd.gradcheck(lambda a, b: OPS.temporal_shift_learnable(a, b, 2, pad, True), (x, w), eps=1e-6, atol=1e-6)
    xd = x.detach()
    for pad in range(5):
        assert torch.autograd.gradcheck(lambda b: OPS.temporal_shift_learnable(xd, b, 2, pad, True), (w,), eps=1e-6, atol=1e-6)


def test_a_second_backward_raises():
    x = torch.randn(4, 3, 2, dtype=torch.float64, requires_grad=True)
    w = torch.tensor([0.3, -0.6, 1.45], dtype=torch.float64, requires_grad=True)
    out = OPS.temporal_shift_learnable(x, w, 2, 0, True)
    gx, = torch.autograd.grad(out.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="double backwards on temporal_shift_learnable not supported"):
        gx.sum().backward()


def test_module_parameters_state_dict_and_the_pair_convention():
    torch.manual_seed(3)
    m = torchshifts.LearnableTemporalShift(4, 6, padding="border", init_shift=2)
    assert [n for n, _ in m.named_parameters()] == ["weight"] and tuple(m.weight.shape) == (6, 1)
    assert float(m.weight.detach().abs().max()) <= 2.0 and list(m.state_dict().keys()) == ["weight"]
    x = torch.randn(8, 6, 3, 3)
    out, loss = m(x)
    assert torch.equal(out, OPS.temporal_shift_learnable(x, m.weight, 4, 1, False))
    assert torch.equal(loss, 5e-4 * m.weight.abs().sum())
    m2 = torchshifts.LearnableTemporalShift(4, 6, padding="border", sparsity_term=0, active_flag=True)
    m2.load_state_dict(m.state_dict())
    out2, loss2 = m2(x)
    assert loss2 is None and torch.equal(out2, OPS.temporal_shift_learnable(x, m.weight, 4, 1, True))
    # it trains: the weight moves with the sparsity loss and the interpolated output's gradient
    opt = torch.optim.SGD(m2.parameters(), lr=0.1)
    before = m2.weight.detach().clone()
    m2(x)[0].square().sum().backward()
    opt.step()
    assert not torch.equal(m2.weight.detach(), before)
    with pytest.raises(AssertionError):
        torchshifts.LearnableTemporalShift(4, 6, padding="nothing")


def test_from_shift_freezes_a_sparse_module():
    torch.manual_seed(4)
    for pad in ("zeros", "border", "periodic", "reflect", "symmetric"):
        m = torchshifts.LearnableTemporalShift(3, 5, padding=pad, init_shift=4)
        with torch.no_grad():
            m.weight[0, 0], m.weight[1, 0] = 0.5, -2.5   # ties: half to even
        frozen = torchshifts.TemporalShift.from_shift(m)
        assert isinstance(frozen, torchshifts.TemporalShift) and not list(frozen.parameters())
        assert torch.equal(frozen.shifts, torch.round(m.weight.detach().reshape(-1)).long()) and frozen.shifts[0] == 0 and frozen.shifts[1] == -2
        x = torch.randn(6, 5, 2, 3)
        go = torch.randn(6, 5, 2, 3)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        m(xa)[0].backward(go)
        out = frozen(xb)
        out.backward(go)
        assert torch.equal(out, m(x)[0]) and torch.equal(xa.grad, xb.grad), pad
    with pytest.raises(ValueError):
        torchshifts.TemporalShift.from_shift(torchshifts.LearnableTemporalShift(3, 5, active_flag=True))
    with pytest.raises(AssertionError):
        torchshifts.TemporalShift.from_shift(torchshifts.Shift1d(5))


def test_argument_checks():
    x = torch.zeros(6, 5, 2)
    w = torch.zeros(5)
    for bad in (lambda: temporal_shift_learnable_func(x, w, 3, 5),                 # padding
                lambda: temporal_shift_learnable_func(x, w, 4),                    # 6 frames are no multiple of 4
                lambda: temporal_shift_learnable_func(x, w, 0),
                lambda: temporal_shift_learnable_func(x, torch.zeros(4), 3),       # channels
                lambda: temporal_shift_learnable_func(x, torch.zeros(5, 2), 3),    # [C, 2]
                lambda: temporal_shift_learnable_func(x, torch.zeros(5, dtype=torch.long), 3),
                lambda: temporal_shift_learnable_func(torch.zeros(6), torch.zeros(6), 3)):
        with pytest.raises(AssertionError):
            bad()
    for bad, text in ((lambda: OPS.temporal_shift_learnable(x, w, 3, 7, False), "padding_mode must be 0..4"),
                      (lambda: OPS.temporal_shift_learnable(x, w, 4, 0, False), "must be a multiple of n_segment"),
                      (lambda: OPS.temporal_shift_learnable(x, torch.zeros(5, 2), 3, 0, False), r"weights must have shape \[C\] or \[C, 1\]"),
                      (lambda: OPS.temporal_shift_learnable(x, torch.zeros(5, dtype=torch.long), 3, 0, False), "weights must be floats"),
                      (lambda: OPS.temporal_shift_learnable(torch.zeros(6), torch.zeros(6), 3, 0, False), "2 to 5 dims")):
        with pytest.raises(RuntimeError, match=text):
            bad()
    # an empty tensor comes back empty, with a zero weight gradient
    e = torch.zeros(0, 5, 2, requires_grad=True)
    we = torch.zeros(5, requires_grad=True)
    out = OPS.temporal_shift_learnable(e, we, 3, 0, True)
    out.sum().backward()
    assert out.shape == e.shape and torch.equal(we.grad, torch.zeros(5))


# ---- SHIFTND_SHIFT_DIM0 at the C ABI, host side only: validation happens before any device work ---------------------------------
def _problem(ndim, dtype, sizes=(2, 5, 3, 8, 1), borders=(0, 3, 0, 8, 0, 1), active=0):
    import ctypes  # noqa: F401
    from torchshifts import abi
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = ndim, dtype, 0, active
    for i, v in enumerate(sizes):
        p.sizes[i] = v
    for i, v in enumerate(borders):
        p.borders[i] = v
    return p


def test_the_flag_at_the_c_abi_host_side():
    import ctypes
    from torchshifts import abi
    INVALID, UNSUPPORTED = -1, -2
    L = abi.lib()
    assert abi.SHIFT_DIM0 == 0x200 and L.shiftnd_abi_version() == 5
    x = torch.empty(2, 5, 3, 8, dtype=torch.bfloat16)
    assert abi.problem(x, 0, False, None).dtype == abi.BF16                     # the defaults leave today's calls as they are
    assert abi.problem(x, 0, False, None, shift_dim0=True).dtype == abi.BF16 | abi.SHIFT_DIM0
    assert abi.problem(x, 0, False, None, w=torch.empty(5), shift_dim0=True).dtype == abi.BF16 | abi.WEIGHTS_F32 | abi.SHIFT_DIM0
    st = (ctypes.c_int64 * 5)(120, 8, 40, 1, 0)
    byref = ctypes.byref

    def forward(p):
        return L.shiftnd_forward(byref(p), None, st, None, None, st, None)

    def backward(p):
        return L.shiftnd_backward(byref(p), None, st, None, st, None, None, st, None, None, 0, None)

    def workspace(p):
        return int(L.shiftnd_backward_workspace_bytes(byref(p)))

    for dt in (abi.F32, abi.F64, abi.F16, abi.BF16, abi.F16 | abi.WEIGHTS_F32, abi.BF16 | abi.WEIGHTS_F32):
        for active in (0, 1):
            ok = _problem(2, dt | abi.SHIFT_DIM0, active=active)
            assert forward(ok) == INVALID and backward(ok) == INVALID              # (NULL tensors; the geometry passed)
            # one (n, c) line's plane fits one workgroup of the walk: N * C partial records of three doubles
            assert workspace(ok) == 2 * 5 * 24
            p1 = _problem(1, dt | abi.SHIFT_DIM0, sizes=(2, 5, 24, 1, 1), borders=(0, 24, 0, 1, 0, 1), active=active)
            assert forward(p1) == INVALID and backward(p1) == INVALID and workspace(p1) == 0       # ndim 1
            cut = _problem(2, dt | abi.SHIFT_DIM0, borders=(1, 3, 0, 8, 0, 1), active=active)
            assert forward(cut) == INVALID and backward(cut) == INVALID and workspace(cut) == 0    # a cut window
            p3 = _problem(3, dt | abi.SHIFT_DIM0, sizes=(2, 5, 3, 4, 2), borders=(0, 3, 0, 4, 0, 2), active=active)
            assert workspace(p3) == 2 * 5 * 24
    # planes of 56 x 56 fp32 = 12544 bytes: two workgroups of 8 KiB per line
    big = _problem(2, abi.F32 | abi.SHIFT_DIM0, sizes=(4, 16, 8, 56 * 56, 1), borders=(0, 8, 0, 56 * 56, 0, 1))
    assert workspace(big) == 4 * 2 * 16 * 24
    for dt in (abi.I8, abi.U8, abi.I32, abi.F32 | abi.WEIGHTS_F32):
        bad = _problem(2, dt | abi.SHIFT_DIM0)
        assert forward(bad) == UNSUPPORTED and backward(bad) == UNSUPPORTED and workspace(bad) == 0
    # the entry points that do not honour the flag refuse it as an unknown dtype
    pool = (ctypes.c_int32 * 2)(2, 2)
    flagged = _problem(2, abi.F32 | abi.SHIFT_DIM0)
    assert L.shiftnd_forward_pooled(byref(flagged), pool, None, None, None, None) == UNSUPPORTED
    assert L.shiftnd_forward_quantized(byref(flagged), None, st, None, abi.U8, 0, 0, None, st, None) == UNSUPPORTED
    # without the flag the same problem answers what it answered
    assert workspace(_problem(2, abi.F32)) >= 2 * 5 * 24
