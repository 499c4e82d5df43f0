"""Mixed precision (fp32 weights with fp16 / bf16 tensors, SHIFTND_WEIGHTS_F32) against the same-dtype kernels the suite already
pins to the oracle: no tolerance anywhere.

Weights that the 16-bit type holds exactly, `w16`, give the same shifts and fractions whether they arrive as `w16` or as
`w16.float()`, so the two calls must run the same kernel, return `out` and `grad_x` bit for bit, and an fp32 `grad_w` that rounds
(RNE, like the same-dtype store) to the same-dtype `grad_w`: it is the same fp64 sum.

Every shape that reaches a kernel family with the knobs untouched (tests/test_routing_gpu.py::FAMILY_ROUTES, by import) runs in
bf16 and in fp16, and so do the shapes of the pooled 16-bit suite (tests/pooled16_cases.py::CASES) through the pooled entry points.

`w` and `grad_w` lie between painted guard bytes (tests/redzone.py) and `grad_w` starts as NaN: a kernel that still stores 2-byte
entries leaves NaN bytes in the fp32 table or differs after rounding, one that reads the fp32 table as 16-bit computes other shifts,
and one that reads a 16-bit table as fp32 runs into the NaN guard behind it.
"""
import pytest
import torch

import pooled16_cases as P
from redzone import Guarded
from test_routing_gpu import FAMILY_ROUTES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BYTE = 0xFF   # repeated: NaN in fp16, bf16 and fp32

FLOAT_ROUTES = [e for e in FAMILY_ROUTES if e[0] in ("forward", "backward")]


def _guarded(values):
    """`values` between two NaN-painted red zones -> the Guarded (its `.t` is the tensor the kernels get)"""
    return Guarded(values.shape, values.dtype, DEV).paint(NAN_BYTE).load(values)


def _grad_w_slot(w):
    """a NaN-filled grad_w of w's shape and dtype between two NaN-painted red zones"""
    return Guarded(w.shape, w.dtype, DEV).paint(NAN_BYTE).poison()


def _assert_grad_w(gw_mixed, gw_same, tdt, what):
    assert gw_mixed.dtype == torch.float32, what
    assert not torch.isnan(gw_mixed).any(), ("fp32 grad_w entries left unwritten", what)
    assert torch.equal(gw_mixed.to(tdt), gw_same), ("grad_w", what, gw_mixed, gw_same)


@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("entry", FLOAT_ROUTES, ids=lambda e: "%s-%s" % (e[0], e[1]))
def test_mixed_equals_same_dtype(entry, tdt):
    from torchshifts import abi
    kind, _, _, shape, cut, pad, active, cl = entry
    nd = len(shape) - 2
    abi.set_path_policy(0)   # (no knob is touched)
    b, new = abi.check_borders(list(shape), cut, nd) if cut else (None, list(shape))
    torch.manual_seed(1)
    x = torch.rand(shape, device=DEV).to(tdt)
    go = torch.rand(new, device=DEV).to(tdt)
    w16 = ((torch.rand(shape[1], nd, device=DEV) * 2 - 1) * 4).to(tdt)
    if cl:
        x, go = abi.to_channels_last(x), abi.to_channels_last(go)
    what = (entry, tdt)
    runs = []
    for w in (w16, w16.float()):
        gw_table = _guarded(w)
        if kind == "forward":
            out = abi.forward(x, gw_table.t, pad, active, b, out=torch.empty_like(go) if cl else None)
            runs.append((abi.last_kernel(), out, None, gw_table, None))
        else:
            slot = _grad_w_slot(w)
            gx, gw = abi.backward(go, gw_table.t, x, pad, active, b, grad_x=torch.empty_like(x) if cl else None, grad_w=slot.t)
            runs.append((abi.last_kernel(), gx, gw, gw_table, slot))
    torch.cuda.synchronize()
    (k_same, t_same, gw_same, _, _), (k_mixed, t_mixed, gw_mixed, _, _) = runs
    assert k_same == k_mixed, ("a mixed problem lands on another kernel", k_same, k_mixed) + what
    assert t_mixed.dtype == tdt and torch.equal(t_mixed, t_same), ("out" if kind == "forward" else "grad_x", k_same) + what
    for _, _, _, table, slot in runs:
        table.assert_intact(("weights", k_same) + what)
        assert torch.equal(table.t, w16.to(table.dtype)), ("weights written", k_same) + what
        if slot is not None:
            slot.assert_intact(("grad_w", k_same) + what)
    if kind == "backward":
        _assert_grad_w(gw_mixed, gw_same, tdt, (k_same,) + what)


def _pooled_or_not_fused(call):
    try:
        return call()
    except RuntimeError as e:
        assert "not served by the fused kernels" in str(e), e
        return None


@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("active", [0, 1], ids=["sparse", "active"])
@pytest.mark.parametrize("ci", range(len(P.CASES)), ids=lambda ci: "case%d" % ci)
def test_mixed_pooled_equals_same_dtype(ci, active, tdt):
    """shiftnd_forward_pooled / shiftnd_backward_pooled: as above under every padding.  A geometry the fused kernels do not serve is
    refused for both kinds of weights alike (SHIFTND_ERR_NOT_FUSED, nothing launched)."""
    from torchshifts import abi
    case = P.CASES[ci]
    nd, shape, pool, _, _ = case
    b, _, pooled = P.geometry(case)
    abi.set_path_policy(0)
    torch.manual_seed(2 + ci)
    x = torch.rand(shape, device=DEV).to(tdt)
    gp = torch.rand(list(shape[:2]) + pooled, device=DEV).to(tdt)
    w16 = ((torch.rand(shape[1], nd, device=DEV) * 2 - 1) * 4).to(tdt)
    served = 0
    for pad in range(5):
        what = (case, pad, active, tdt)
        fwd, bwd = [], []
        for w in (w16, w16.float()):
            table, slot = _guarded(w), _grad_w_slot(w)
            out = _pooled_or_not_fused(lambda: abi.forward_pooled(x, table.t, pad, active, pool, b))
            fwd.append((out, abi.last_kernel() if out is not None else None))
            res = _pooled_or_not_fused(lambda: abi.backward_pooled(gp, table.t, x, pad, active, pool, b, grad_w=slot.t))
            bwd.append((res, abi.last_kernel() if res is not None else None))
            torch.cuda.synchronize()
            table.assert_intact(("weights",) + what)
            slot.assert_intact(("grad_w",) + what)
        (o_same, kf_same), (o_mixed, kf_mixed) = fwd
        assert kf_same == kf_mixed, ("forward kernels", kf_same, kf_mixed) + what
        if o_same is not None:
            served += 1
            assert o_mixed.dtype == tdt and torch.equal(o_mixed, o_same), ("pooled out", kf_same) + what
        (r_same, kb_same), (r_mixed, kb_mixed) = bwd
        assert kb_same == kb_mixed, ("backward kernels", kb_same, kb_mixed) + what
        if r_same is not None:
            served += 1
            assert r_mixed[0].dtype == tdt and torch.equal(r_mixed[0], r_same[0]), ("grad_x", kb_same) + what
            _assert_grad_w(r_mixed[1], r_same[1], tdt, (kb_same,) + what)
    assert served > 0, ("no padding of this case reached a fused kernel", case)
