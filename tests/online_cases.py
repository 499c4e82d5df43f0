"""What the online temporal shift tests share: the reference, the tables and the step loop.

The reference is the definition in the README: T online steps on the frames of a clip-major tensor X = [B * T, C, ...] give, stacked,
temporal_shift_func(X, shifts, T, padding_mode) -- which is the oracle's 2-D sparse forward (oracle.oracle, pinned to the reference)
of the [B, C, T, M] view under the table (s, 0), the way inplace_cases.reference builds it.  Never the code under test."""
import numpy as np
import torch

import inplace_cases as IC
from inplace_cases import F16, BF16, F32, F64, U8, I8, I32, same_bits, data  # noqa: F401

T = 5
WRAP = torch.tensor([1, 0, 2, 0, 3])   # D = 3 with T = 5: the rotation wraps


def default_table(C, fold_div=8):
    """the uni-directional table: the first C // fold_div channels one frame late"""
    s = torch.zeros(C, dtype=torch.int64)
    s[:C // fold_div] = 1
    return s


def causal_table(rs, C, D):
    """shifts from [0, D] with 0 and D always present where C allows"""
    s = rs.randint(0, D + 1, size=C)
    s[[0, C - 1][:C]] = [D, 0][:C]
    return torch.from_numpy(s.astype(np.int64))


def runs_table(C, D):
    """constant over runs of 8 channels: uniform channels-last pieces"""
    s = torch.zeros(C, dtype=torch.int64)
    for k, v in enumerate((1, 0, D, 2)):
        s[8 * k:8 * (k + 1)] = min(v, D)
    return s


def clip(rs, B, C, spatial, dtype, steps=T):
    """X [B * steps, C, *spatial] (clip-major) and its frames [steps][B, C, *spatial] (contiguous copies)"""
    X = data(rs, (B * steps, C) + tuple(spatial), dtype)
    frames = X.view(B, steps, C, *spatial)
    return X, [frames[:, t].contiguous() for t in range(steps)]


def reference_frames(X, shifts, steps, pad, zero_point=0):
    """the oracle's answer for every step: [steps][B, C, *spatial]"""
    want = IC.reference(X, shifts, steps, pad, zero_point)
    want = want.view(X.shape[0] // steps, steps, *X.shape[1:])
    return [want[:, t].contiguous() for t in range(steps)]


def expected_state(frames, shifts, initial):
    """the state after len(frames) steps, from the definition: slot k of channel c holds frame T-1-k for k < s_c (the initial slot
    when the stream is younger than that), and its initial bytes for k >= s_c.  `initial`: the initial state [D, B, C, ...]"""
    want = initial.clone()
    n = len(frames)
    for c, s in enumerate(shifts.tolist()):
        for k in range(min(s, initial.shape[0])):
            if n - 1 - k >= 0:
                want[k][:, c] = frames[n - 1 - k][:, c]
            else:   # the stream is younger: the initial slots have moved on by n places
                want[k][:, c] = initial[k - n][:, c]
    return want


def layout(t, channels_last):
    """a frame (or any [B, C, ...] tensor) in the contiguous or the dense channels-last layout"""
    if not channels_last:
        return t.contiguous()
    order = [0] + list(range(2, t.dim())) + [1]
    back = [0, t.dim() - 1] + list(range(1, t.dim() - 1))
    return t.permute(order).contiguous().permute(back)


def quantized(int_repr, zp, channels_last=False, scale=0.05):
    if not channels_last:
        return torch._make_per_tensor_quantized_tensor(int_repr.contiguous(), scale, zp)
    order = [0] + list(range(2, int_repr.dim())) + [1]
    back = [0, int_repr.dim() - 1] + list(range(1, int_repr.dim() - 1))
    return torch._make_per_tensor_quantized_tensor(int_repr.permute(order).contiguous(), scale, zp).permute(back)
