"""SHIFTND_WEIGHTS_F32 (fp32 weights with fp16 / bf16 tensors) at the C ABI, host side only: which dtypes take the flag, which
forms refuse it, and that the answers which do not depend on the weights' type stay what they are.  Nothing here touches a device:
argument validation happens before any device work (as tests/test_abi_symbols.py::test_host_only_entry_points)."""
import ctypes

import pytest
import torch

from torchshifts import abi

INVALID, UNSUPPORTED = -1, -2


def _problem(ndim, dtype, sizes=(2, 3, 8, 16, 1), borders=(0, 8, 0, 16, 0, 1)):
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = ndim, dtype, 0, 0
    for i, v in enumerate(sizes):
        p.sizes[i] = v
    for i, v in enumerate(borders):
        p.borders[i] = v
    return p


def test_flag_value():
    assert abi.WEIGHTS_F32 == 0x100
    # ... and the wrappers derive it from the weights: fp32 weights with a 16-bit tensor, and with nothing else
    x16, x32 = torch.empty(1, 2, 4, 8, dtype=torch.bfloat16), torch.empty(1, 2, 4, 8)
    w32, w16 = torch.empty(2, 2), torch.empty(2, 2, dtype=torch.bfloat16)
    assert abi.problem(x16, 0, False, None, w=w32).dtype == abi.BF16 | abi.WEIGHTS_F32
    assert abi.problem(x16.half(), 0, False, None, w=w32).dtype == abi.F16 | abi.WEIGHTS_F32
    assert abi.problem(x16, 0, False, None, w=w16).dtype == abi.BF16
    assert abi.problem(x32, 0, False, None, w=w32).dtype == abi.F32
    assert abi.problem(x16, 0, False, None).dtype == abi.BF16


@pytest.mark.parametrize("dtype", [abi.F32, abi.F64, abi.I8])
def test_flag_on_other_dtypes_is_unsupported(dtype):
    L = abi.lib()
    st = (ctypes.c_int64 * 5)()
    p = _problem(2, dtype | abi.WEIGHTS_F32)
    assert L.shiftnd_forward(ctypes.byref(p), None, st, None, None, st, None) == UNSUPPORTED
    assert L.shiftnd_backward(ctypes.byref(p), None, st, None, st, None, None, st, None, None, 0, None) == UNSUPPORTED
    pool = (ctypes.c_int32 * 2)(2, 2)
    assert L.shiftnd_forward_pooled(ctypes.byref(p), pool, None, None, None, None) == UNSUPPORTED
    assert L.shiftnd_backward_pooled(ctypes.byref(p), pool, None, None, None, None, None, None, 0, None) == UNSUPPORTED
    assert L.shiftnd_pooled_sizes(ctypes.byref(p), pool, (ctypes.c_int64 * 3)()) == UNSUPPORTED


@pytest.mark.parametrize("dtype", [abi.I8, abi.U8, abi.I32])
def test_flag_on_the_quantized_entry_points_is_unsupported(dtype):
    L = abi.lib()
    st = (ctypes.c_int64 * 5)()
    p = _problem(2, dtype | abi.WEIGHTS_F32)
    assert L.shiftnd_forward_quantized(ctypes.byref(p), None, st, None, abi.U8, 0, 0, None, st, None) == UNSUPPORTED
    pool = (ctypes.c_int32 * 2)(2, 2)
    assert L.shiftnd_forward_quantized_pooled(ctypes.byref(p), pool, None, None, abi.U8, 0, 0, 0, None, None) == UNSUPPORTED


@pytest.mark.parametrize("dtype", [abi.F16, abi.BF16])
def test_geometry_is_validated_behind_the_flag(dtype):
    L = abi.lib()
    st = (ctypes.c_int64 * 5)()
    p = _problem(7, dtype | abi.WEIGHTS_F32)
    assert L.shiftnd_forward(ctypes.byref(p), None, st, None, None, st, None) == INVALID
    # a valid, non-empty problem with NULL tensors: still the flag-free answer
    p = _problem(2, dtype | abi.WEIGHTS_F32)
    assert L.shiftnd_forward(ctypes.byref(p), None, st, None, None, st, None) == INVALID


@pytest.mark.parametrize("dtype", [abi.F16, abi.BF16])
def test_flag_with_the_input_free_forms_is_invalid(dtype):
    """x == NULL && grad_w == NULL (the fixed ops' grad_x-only backward) takes a table of the tensors' type only"""
    L = abi.lib()
    st = (ctypes.c_int64 * 5)()
    p = _problem(2, dtype | abi.WEIGHTS_F32)
    assert L.shiftnd_backward(ctypes.byref(p), None, st, None, st, None, None, st, None, None, 0, None) == INVALID
    assert L.shiftnd_backward(ctypes.byref(p), None, st, None, None, None, None, st, None, None, 0, None) == INVALID
    pool = (ctypes.c_int32 * 2)(2, 2)
    assert L.shiftnd_backward_pooled(ctypes.byref(p), pool, None, None, None, None, None, None, 0, None) == INVALID


GEOMETRIES = [   # ndim, sizes, borders, pool
    (2, (2, 3, 18, 32, 1), (0, 18, 0, 32, 0, 1), (2, 2)),
    (3, (1, 2, 6, 9, 40), (1, 5, 1, 8, 1, 39), (2, 2, 2)),
    (1, (2, 3, 4096, 1, 1), (0, 4096, 0, 1, 0, 1), (2,)),
]


@pytest.mark.parametrize("active", [0, 1])
@pytest.mark.parametrize("dtype", [abi.F16, abi.BF16])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dd" % g[0])
def test_workspace_and_sizes_do_not_depend_on_the_flag(geometry, dtype, active):
    L = abi.lib()
    ndim, sizes, borders, pool = geometry
    plain, mixed = _problem(ndim, dtype, sizes, borders), _problem(ndim, dtype | abi.WEIGHTS_F32, sizes, borders)
    plain.active = mixed.active = active
    k = (ctypes.c_int32 * ndim)(*pool)
    a, b = (int(L.shiftnd_backward_workspace_bytes(ctypes.byref(p))) for p in (plain, mixed))
    assert a == b and a > 0, (a, b)
    a, b = (int(L.shiftnd_backward_pooled_workspace_bytes(ctypes.byref(p), k)) for p in (plain, mixed))
    assert a == b and a > 0, (a, b)
    got = []
    for p in (plain, mixed):
        sp = (ctypes.c_int64 * 3)()
        assert L.shiftnd_pooled_sizes(ctypes.byref(p), k, sp) == 0
        got.append(list(sp))
    assert got[0] == got[1]
    # the flag on a dtype that does not take it: the queries that return no status answer 0
    bad = _problem(ndim, abi.F32 | abi.WEIGHTS_F32, sizes, borders)
    assert int(L.shiftnd_backward_workspace_bytes(ctypes.byref(bad))) == 0
    assert int(L.shiftnd_backward_pooled_workspace_bytes(ctypes.byref(bad), k)) == 0
