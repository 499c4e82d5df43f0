"""Exact-data and single-tap parity of the channels-last kernels on fp16 / bf16 tensors: the LDS-tiled NHWC / NDHWC kernels serve the
tensors as they lie (csrc/shiftnd_cl_tiled.hip, shiftnd_cl_tiled3.hip), under policy 4 with the tiled kernels off the channel-fastest
ones (csrc/shiftnd_cl.hip).  Fixtures, reference and assertion functions: tests/exact16_cases.py, as tests/test_exact16_gpu.py.

Input, output and grad_x are channels-last (abi.to_channels_last); the incoming gradient is channels-last or NCHW / NCDHW-contiguous.
With C = 64 / 16 the fixture's special weights sit in the first three channels and drawn quarter / half weights in the rest, across
the 8-channel lane groups.  The dense exact calls run again with one row per band (knob 21 = 1).  Every padding and both shifts."""
import pytest
import torch

import exact16_cases as EC
from test_exact16_gpu import DEV, _reset, abi, dev, host, nan_like   # noqa: F401  (abi: the fixture)

pytestmark = pytest.mark.gpu


def run_cl_case(abi, ci, dt, kind, seen):
    case = EC.CL_CASES[ci]
    nd, shape, cut = case[:3]
    tdt = EC.DTYPES[dt]
    x, w, grads = EC._inputs(1, ci, dt if kind == "random" else "", kind)
    b, win = EC.geometry(case)
    xd, wd = abi.to_channels_last(dev(x, tdt)), dev(w, tdt)
    gds = [dev(g, tdt) for g in grads]
    gcl = [abi.to_channels_last(g) for g in gds]
    out_nan = nan_like(abi.to_channels_last(torch.empty(win, dtype=tdt, device=DEV)))
    gx_nan = nan_like(xd)
    for pad, active in EC.SWEEP:
        what = (shape, cut, dt, kind, pad, active)
        r = EC.reference(ci, dt, kind, pad, active, 1)

        def forward(tag, want):
            out = abi.forward(xd, wd, pad, active, b, out=out_nan.clone())
            name = abi.last_kernel()
            assert out.stride() == out_nan.stride() and name == want, what + (tag, name, want)
            seen.add(name)
            EC.check_forward(host(out, tdt), r, active, kind, tdt, what + (tag, name))

        def backward(k, grad, tag, want):
            gx, gw = abi.backward(grad, wd, xd, pad, active, b, grad_x=gx_nan.clone())
            name = abi.last_kernel()
            assert name == want, what + (tag, "call %d" % k, name, want)
            seen.add(name)
            EC.check_backward(host(gx, tdt), host(gw, tdt), r["calls"][k], active, kind, tdt, what + (tag, "call %d" % k, name))

        def calls(tag, plain=False):
            forward(tag, EC.CL_PLAIN["f%d" % active] if plain else EC.cl_expected(case, "f", active))
            for k in range(len(gds)):
                backward(k, gcl[k], tag, EC.CL_PLAIN["b%d" % active] if plain else EC.cl_expected(case, "b", active, True))
                if not plain:
                    backward(k, gds[k], tag + " contiguous gradient", EC.cl_expected(case, "b", active, False))

        calls("default")
        if kind != "exact":
            continue
        try:
            abi.set_tuning(21, 1)   # one row per band
            calls("knob 21 = 1")
        finally:
            _reset(abi)
        try:
            abi.set_path_policy(4)
            abi.set_tuning(20, 0)
            abi.set_tuning(23, 1)
            calls("policy 4", plain=True)
        finally:
            _reset(abi)


@pytest.mark.parametrize("kind", ["exact", "probe", "random"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_channels_last(abi, dt, kind):
    seen = set()
    for ci in range(len(EC.CL_CASES)):
        run_cl_case(abi, ci, dt, kind, seen)
    if kind == "exact":
        print("served (%s):" % dt, sorted(seen))
        assert EC.CL_SERVED <= seen, sorted(EC.CL_SERVED - seen)
