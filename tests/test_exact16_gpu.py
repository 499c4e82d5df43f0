"""Exact-data and single-tap parity of the unpooled kernels on fp16 / bf16 tensors (fp32 as a control), through the C ABI
(shiftnd_forward / shiftnd_backward), against the CPU oracle on widened values.  Table, fixtures, reference, alternates and assertion
functions: tests/exact16_cases.py (their own self-checks, without a GPU: tests/test_exact16_cases.py).

  exact data ........ out, grad_x and grad_w == round16(gw64) bit for bit (fp32: grad_w == the fp64 oracle's)
  probe data ........ the same, the gradient one +-1 per (n, c) plane at the piece boundaries and both ends of the window
  random data ....... the sparse shift: out and grad_x bit for bit; the interpolating shift: 1 ulp (+ FLOOR16) per element;
                      grad_w per entry within 0.51 ulp16(gw64) + 1e-5 max|gw64|
  routes ............ the kernel name of every default-route 16-bit call against the table
  alternates ........ the dense exact calls again under every path policy and knob of exact16_cases.ALTERNATES: the reference's bits,
                      or the ABI's RuntimeError where the policy does not serve the problem

Outputs are handed over filled with NaN: an element no kernel wrote fails.  Every padding 0-4 and both shifts on every case."""
import numpy as np
import pytest
import torch

import exact16_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _reset(A):
    A.set_path_policy(0)
    for k, v in EC.KNOB_DEFAULTS.items():
        A.set_tuning(k, v)


@pytest.fixture()
def abi():
    from torchshifts import abi as A
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    _reset(A)
    yield A
    _reset(A)


def dev(a, tdt):
    return torch.from_numpy(np.array(a)).to(tdt).to(DEV)   # (a copy: the shared references are read-only)


def host(t, tdt):
    """widened values; fp32 grad_w stays fp32 (compared with the fp64 oracle as it is)"""
    return t.float().cpu().numpy() if tdt != torch.float32 else t.cpu().numpy()


def nan_like(t):
    return torch.full_like(t, float("nan"))


class Log:
    """what the runs saw: kernel names per direction, the alternates' routes, the calls a policy refused"""

    def __init__(self):
        self.forward, self.backward, self.moved, self.refused = set(), set(), {}, 0

    def note(self, direction, name):
        (self.forward if direction == "f" else self.backward).add(name)


def run_case(abi, ci, dt, kind, log, check=True, alternates=False):
    """every padding and shift of CASES[ci] on the default route (kernel names asserted for 16-bit tensors); with `alternates` the
    same calls again under every entry of EC.ALTERNATES.  check=False: routes only."""
    case = EC.CASES[ci]
    nd, shape, cut = case[:3]
    tdt = EC.DTYPES[dt]
    dkey = dt if kind == "random" else ""
    x, w, grads = EC._inputs(0, ci, dkey, kind)
    b, win = EC.geometry(case)
    xd, wd = dev(x, tdt), dev(w, tdt)
    gds = [dev(g, tdt) for g in grads]
    out_nan, gx_nan = torch.full(win, float("nan"), dtype=tdt, device=DEV), nan_like(xd)
    for pad, active in EC.SWEEP:
        what = (shape, cut, dt, kind, pad, active)
        r = EC.reference(ci, dt, kind, pad, active) if check else None

        def forward(tag):
            out = abi.forward(xd, wd, pad, active, b, out=out_nan.clone())
            name = abi.last_kernel()
            if check:
                EC.check_forward(host(out, tdt), r, active, kind, tdt, what + (tag, name))
            return name

        def backward(k, tag):
            gx, gw = abi.backward(gds[k], wd, xd, pad, active, b, grad_x=gx_nan.clone())
            name = abi.last_kernel()
            if check:
                EC.check_backward(host(gx, tdt), host(gw, tdt), r["calls"][k], active, kind, tdt, what + (tag, "call %d" % k, name))
            return name

        names = {"f": forward("default")}
        for k in range(len(gds)):
            names["b"] = backward(k, "default")
            for d in "fb":
                log.note(d, names[d])
                if tdt != torch.float32:
                    assert names[d] == EC.expected(case, d, active, pad), what + (d, names[d], EC.expected(case, d, active, pad))
        if not alternates:
            continue
        for knob, value in EC.ALTERNATES:
            try:
                if knob == "policy":
                    abi.set_path_policy(value)
                else:
                    abi.set_tuning(knob, value)
                for d, call in (("f", lambda: forward((knob, value))), ("b", lambda: backward(0, (knob, value)))):
                    try:
                        name = call()
                    except RuntimeError as e:   # this policy does not serve the problem (nothing was launched): counts for nothing
                        if "invalid argument" not in str(e):
                            raise
                        log.refused += 1
                        continue
                    log.note(d, name)
                    if name != names[d]:
                        log.moved.setdefault((shape, str(cut), d, active, names[d], name), set()).add((knob, value, pad))
            finally:
                _reset(abi)


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_exact_data(abi, dt, nd):
    """dyadic inputs: every intermediate is exact, so the kernels must return the reference's bits whatever their evaluation order,
    under the default route and under every policy and knob"""
    log = Log()
    for ci in EC.group(nd):
        run_case(abi, ci, dt, "exact", log, alternates=True)
    assert log.forward and log.backward


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_probe_data(abi, dt, nd):
    """one +-1 per (n, c) plane: each position counted once, with the right corner weights, bit for bit in bf16 too"""
    log = Log()
    for ci in EC.group(nd):
        run_case(abi, ci, dt, "probe", log)
    assert log.backward


@pytest.mark.parametrize("nd", [1, 2, 3])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_random_data(abi, dt, nd):
    """uniform inputs under per-element bars derived from the number formats"""
    log = Log()
    for ci in EC.group(nd):
        run_case(abi, ci, dt, "random", log)
    assert log.backward


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_16bit_served_set(abi, dt):
    """the 16-bit runs of the table (the calls of test_exact_data, routes only) reach every unpooled kernel family of contiguous
    tensors: a route that silently moves shows up here as well as at its call"""
    log = Log()
    for ci in range(len(EC.CASES)):
        run_case(abi, ci, dt, "exact", log, check=False, alternates=True)
    print("backward (%s):" % dt, sorted(log.backward))
    print("forward (%s):" % dt, sorted(log.forward))
    for key, how in sorted(log.moved.items(), key=str):
        print("moved:", key, sorted(how, key=str))
    assert EC.SERVED_BACKWARD <= log.backward, sorted(EC.SERVED_BACKWARD - log.backward)
    assert EC.SERVED_FORWARD <= log.forward, sorted(EC.SERVED_FORWARD - log.forward)
    for names in EC.SERVED_BACKWARD_ANY:
        assert log.backward & set(names), names
    for names in EC.SERVED_FORWARD_ANY:
        assert log.forward & set(names), names
