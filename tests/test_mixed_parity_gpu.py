"""Mixed precision against the oracle: fp32 weights that 16 bits cannot hold, with fp16 / bf16 tensors.

The reference is the fp32 oracle on the widened tensors and the fp32 weights as they are (the way tests/test_hip_parity.py builds
its 16-bit references, with nothing rounded on the weights' side), gw64 the fp64 oracle on the same values.  Bars:
  sparse shift ........ out and grad_x bit for bit after the one RNE rounding (they are copies)
  interpolating ....... out and grad_x within 1 ulp of the 16-bit type per element (+ FLOOR16, the absolute floor the suite grants
                        16-bit interpolation of data in [-1, 1] wherever it compares per element: pooled16_cases.assert_ulp_close)
  grad_w (fp32) ....... rel_err < 1e-5 of gw64, and every entry within 1e-5 max|gw64|: the project's fp32 bars -- the arithmetic is
                        the fp32 path's on widened data, and nothing is narrowed to 16 bits

The differential cases at the end are the ones a silent `weights.to(x.dtype)` fails: 1.498 is 1.5 in bf16 (a shift of 2, not 1),
-2.502 is -2.5 (-2, not -3), and 301 is 300 or 302.
"""
import functools

import numpy as np
import pytest
import torch

import pooled16_cases as P
from cases import rel_err
from oracle import oracle as O
from test_hip_parity import _weights
from test_step_gpu import FLOOR16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the smallest shapes that still reach the main families: step / flat / crop (2-D), walk16 and its cropped form (3-D), rows (1-D)
SHAPES = [
    ((2, 3, 16, 32), None),
    ((2, 2, 7, 11), None),
    ((2, 3, 18, 34), [[1, 1], [1, 1]]),
    ((1, 2, 32, 7, 200), None),
    ((1, 2, 6, 9, 40), [[1, 1], [1, 1], [1, 1]]),
    ((2, 3, 4096), None),
]
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


@functools.lru_cache(maxsize=None)
def _inputs(si, dt):
    """x, go (values of the 16-bit type, as fp32 arrays), w (fp32, NOT representable in 16 bits), borders -- drawn once, read-only"""
    shape, cut = SHAPES[si]
    nd = len(shape) - 2
    tdt = DTYPES[dt]
    rs = np.random.RandomState(1000 + 10 * si + (dt == "f16"))
    b, new = O.check_borders(list(shape), cut, nd)
    x = P.round16(rs.uniform(-1, 1, size=shape), tdt)
    go = P.round16(rs.uniform(-1, 1, size=new), tdt)
    w = _weights(rs, shape[1], nd, shape[2:]).astype(np.float32)
    w[-1, :] = [1.498, -2.502, 0.7512][:nd]   # (the last channel: values bf16 moves across a rounding boundary)
    assert not P.representable(w, tdt)
    for a in (x, go, w):
        a.setflags(write=False)
    return x, go, w, b


@functools.lru_cache(maxsize=None)
def _reference(si, dt, pad, active):
    x, go, w, b = _inputs(si, dt)
    tdt = DTYPES[dt]
    out = P.round16(O.forward(x, w, pad, active, b), tdt)
    gx = P.round16(O.backward(go, w, x, pad, active, b)[0], tdt)
    _, gw64 = O.backward(go.astype(np.float64), w.astype(np.float64), x.astype(np.float64), pad, active, b)
    for a in (out, gx, gw64):
        a.setflags(write=False)
    return out, gx, gw64


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("active", [0, 1], ids=["sparse", "active"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=lambda si: "x".join(map(str, SHAPES[si][0])) + ("cut" if SHAPES[si][1] else ""))
def test_mixed_vs_oracle(si, active, dt):
    from torchshifts import abi
    abi.set_path_policy(0)
    tdt = DTYPES[dt]
    x, go, w, b = _inputs(si, dt)
    xd, god = (torch.from_numpy(a.copy()).to(tdt).to(DEV) for a in (x, go))   # (the cached arrays are read-only)
    wd = torch.from_numpy(w.copy()).to(DEV)
    assert wd.dtype == torch.float32
    for pad in range(5):
        ref_out, ref_gx, gw64 = _reference(si, dt, pad, active)
        out = abi.forward(xd, wd, pad, active, b)
        kf = abi.last_kernel()
        gx, gw = abi.backward(god, wd, xd, pad, active, b)
        kb = abi.last_kernel()
        what = (SHAPES[si], dt, pad, active, kf, kb)
        assert out.dtype == tdt and gx.dtype == tdt and gw.dtype == torch.float32, what
        out, gx, gw = out.float().cpu().numpy(), gx.float().cpu().numpy(), gw.cpu().numpy()
        if not active:
            P.assert_bits(out, ref_out, what + ("forward",))
            P.assert_bits(gx, ref_gx, what + ("grad_x",))
        else:
            P.assert_ulp_close(out, ref_out, tdt, FLOOR16, what + ("forward",))
            P.assert_ulp_close(gx, ref_gx, tdt, FLOOR16, what + ("grad_x",))
        err = rel_err(gw, gw64)
        worst = np.abs(gw.astype(np.float64) - gw64).max()
        print("grad_w", what, "rel_err %.3g" % err, "worst entry %.3g of bound %.3g" % (worst, 1e-5 * np.abs(gw64).max()))
        assert err < 1e-5, what + ("grad_w", err)
        assert (np.abs(gw.astype(np.float64) - gw64) <= 1e-5 * np.abs(gw64).max()).all() and not np.isnan(gw).any(), what + ("grad_w entries",)


# ---- what a silent weights.to(x.dtype) fails --------------------------------------------------------------------------------
@pytest.mark.parametrize("wv,shift,shift16", [(1.498, 1, 2), (-2.502, -3, -2)])
def test_fp32_weight_is_not_rounded_to_bf16(wv, shift, shift16):
    """sparse shift on bf16 (1, 2, 8, 64), periodic: the result is the roll by rint(w) of the fp32 weight -- and NOT what the
    same-dtype call under w.to(bf16) returns, which rounds the weight across .5 first"""
    from torchshifts import abi
    abi.set_path_policy(0)
    torch.manual_seed(5)
    x = torch.rand(1, 2, 8, 64, device=DEV).to(torch.bfloat16)
    w = torch.full((2, 2), wv, device=DEV, dtype=torch.float32)
    assert float(w.to(torch.bfloat16)[0, 0]) == (1.5 if wv > 0 else -2.5)
    mixed = abi.forward(x, w, 2, 0)
    same = abi.forward(x, w.to(torch.bfloat16), 2, 0)
    assert torch.equal(mixed, torch.roll(x, (shift, shift), (2, 3))), (wv, shift)
    assert torch.equal(same, torch.roll(x, (shift16, shift16), (2, 3))), (wv, shift16)
    assert not torch.equal(mixed, same)
    # ... and the backward follows the same shift: grad_x of the sparse shift is the gradient rolled back
    go = torch.rand(1, 2, 8, 64, device=DEV).to(torch.bfloat16)
    gx, gw = abi.backward(go, w, x, 2, 0)
    assert gw.dtype == torch.float32
    assert torch.equal(gx, torch.roll(go, (-shift, -shift), (2, 3))), (wv, shift)


def test_fp32_weight_beyond_bf16_integers():
    """w = 301 (bf16 holds 300 and 302) on bf16 (1, 1, 1024), periodic: a roll by exactly 301"""
    from torchshifts import abi
    abi.set_path_policy(0)
    torch.manual_seed(6)
    x = torch.rand(1, 1, 1024, device=DEV).to(torch.bfloat16)
    w = torch.full((1, 1), 301.0, device=DEV, dtype=torch.float32)
    assert float(w.to(torch.bfloat16)) != 301.0
    for active in (0, 1):   # (an integral weight interpolates with fraction 0: the same roll)
        assert torch.equal(abi.forward(x, w, 2, active), torch.roll(x, 301, 2)), active
