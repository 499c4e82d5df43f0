"""Functional interface: shift{1,2,3}d_func (same names, arguments and checks as the reference's
torchshifts/functional.py:7-99).  Each call validates its arguments with `assert` (AssertionError,
like the reference) and forwards to the dispatcher op `torch.ops.torchshifts.shift{N}d`, which on a
HIP tensor runs the gfx950 kernels of libshiftnd_hip.so.
"""
from typing import Optional

import torch

from .extension import _assert_has_ops

Tensor = torch.Tensor

_PADDING_DOC = "0 - zeros, 1 - border, 2 - periodic, 3 - reflect, 4 - symmetric"


def _shift_func(dim: int, input: Tensor, weights: Tensor, padding_mode: int, active_flag: bool,
                borders: Optional[Tensor], pool=None) -> Tensor:
    name = f"shift{dim}d_func()" if pool is None else f"shift{dim}d_pool_func()"
    _assert_has_ops()
    assert padding_mode in [0, 1, 2, 3, 4], f"{name} expected padding_mode can be {_PADDING_DOC}"
    assert len(input.shape) == dim + 2, f"{name}: expected {dim + 2}D tensor as input, but it is shape is {input.shape}"
    assert weights.shape[-1] == dim, \
        f"{name}: expected [n_channels,{dim}] tensor as weight, but it is shape is {weights.shape}"
    assert input.shape[1] == weights.shape[0], \
        (f"{name}: expected that input and weight have equal number of channels, but input have "
         f"{input.shape[1]} and weight have {weights.shape[0]} channels.")
    assert input.device == weights.device, \
        (f"{name}: expected input and weights to be on same device, but input is  on {input.device} "
         f"and weights is on {weights.device}")
    if borders is not None:
        assert (len(borders.shape) == 2) and (borders.shape[1] == 2) and (borders.shape[0] == dim), \
            f"borders must have shape [{dim}, 2]"
    else:
        borders = torch.Tensor()
    if pool is not None:
        if isinstance(pool, torch.Tensor):
            pool = pool.reshape(-1).tolist()
        pool = [int(pool)] * dim if isinstance(pool, (int, float)) else [int(k) for k in pool]
        assert len(pool) == dim and all(k >= 1 for k in pool), f"{name}: pool must be {dim} window sizes >= 1"
        return getattr(torch.ops.torchshifts, f"shift{dim}d_pool")(input, weights, borders, pool, padding_mode, active_flag)
    return getattr(torch.ops.torchshifts, f"shift{dim}d")(input, weights, borders, padding_mode, active_flag)


def shift1d_func(input: Tensor, weights: Tensor, padding_mode: int, active_flag: bool,
                 borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H] tensor; weights [C, 1]; borders [1, 2] = (cut_left, cut_right)."""
    return _shift_func(1, input, weights, padding_mode, active_flag, borders)


def shift2d_func(input: Tensor, weights: Tensor, padding_mode: int, active_flag: bool,
                 borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H, W] tensor; weights [C, 2] (H, W); borders [2, 2]."""
    return _shift_func(2, input, weights, padding_mode, active_flag, borders)


def shift3d_func(input: Tensor, weights: Tensor, padding_mode: int, active_flag: bool,
                 borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H, W, D] tensor; weights [C, 3] (H, W, D); borders [3, 2]."""
    return _shift_func(3, input, weights, padding_mode, active_flag, borders)


# ---- shift + average pool as one op (not in the reference) -----------------------
# `pool` is the window (= stride) per spatial dim, an int or a list.  The result equals
# avg_pool{N}d(shift{N}d_func(...), kernel_size=pool, stride=pool, ceil_mode=True), the tail the reference's
# modules attach when they emulate a strided depthwise conv (modules/shifts.py:81-89, 150-153).  On HIP tensors
# the full-size shift output is never written to memory; on CPU tensors the op is literally that sequence.
def shift1d_pool_func(input: Tensor, weights: Tensor, padding_mode: int, active_flag: bool,
                      borders: Optional[Tensor] = None, pool=2) -> Tensor:
    return _shift_func(1, input, weights, padding_mode, active_flag, borders, pool)


def shift2d_pool_func(input: Tensor, weights: Tensor, padding_mode: int, active_flag: bool,
                      borders: Optional[Tensor] = None, pool=2) -> Tensor:
    return _shift_func(2, input, weights, padding_mode, active_flag, borders, pool)


def shift3d_pool_func(input: Tensor, weights: Tensor, padding_mode: int, active_flag: bool,
                      borders: Optional[Tensor] = None, pool=2) -> Tensor:
    return _shift_func(3, input, weights, padding_mode, active_flag, borders, pool)


# ---- fixed (grouped) shifts: integer shifts that nobody learns (not in the reference) -----------------------------------
# `shifts` is a [n_channels, dim] table of integers (int32 / int64, or floats that hold integers; a float table is rounded half
# to even like the sparse shift's weights).  The result equals shift{N}d_func(input, shifts.to(input.dtype), padding_mode, False,
# borders); the backward returns the input gradient alone -- the autograd node keeps the table, not the input, and on HIP tensors
# no kernel reads the input or forms a weight gradient.  The table is converted to the input's dtype: exact for |shift| <= 256
# in bfloat16, <= 2048 in float16.
def _shift_fixed_func(dim: int, input: Tensor, shifts: Tensor, padding_mode: int, borders: Optional[Tensor], pool=None) -> Tensor:
    name = f"shift{dim}d_fixed_func()" if pool is None else f"shift{dim}d_fixed_pool_func()"
    _assert_has_ops()
    assert padding_mode in [0, 1, 2, 3, 4], f"{name} expected padding_mode can be {_PADDING_DOC}"
    assert len(input.shape) == dim + 2, f"{name}: expected {dim + 2}D tensor as input, but it is shape is {input.shape}"
    assert len(shifts.shape) == 2 and shifts.shape[-1] == dim, \
        f"{name}: expected [n_channels,{dim}] tensor as shifts, but it is shape is {shifts.shape}"
    assert input.shape[1] == shifts.shape[0], \
        (f"{name}: expected that input and shifts have equal number of channels, but input have "
         f"{input.shape[1]} and shifts have {shifts.shape[0]} channels.")
    assert input.device == shifts.device, \
        (f"{name}: expected input and shifts to be on same device, but input is  on {input.device} "
         f"and shifts is on {shifts.device}")
    if borders is not None:
        assert (len(borders.shape) == 2) and (borders.shape[1] == 2) and (borders.shape[0] == dim), \
            f"borders must have shape [{dim}, 2]"
    else:
        borders = torch.Tensor()
    if pool is not None:
        if isinstance(pool, torch.Tensor):
            pool = pool.reshape(-1).tolist()
        pool = [int(pool)] * dim if isinstance(pool, (int, float)) else [int(k) for k in pool]
        assert len(pool) == dim and all(k >= 1 for k in pool), f"{name}: pool must be {dim} window sizes >= 1"
        return getattr(torch.ops.torchshifts, f"shift{dim}d_fixed_pool")(input, shifts, borders, pool, padding_mode)
    return getattr(torch.ops.torchshifts, f"shift{dim}d_fixed")(input, shifts, borders, padding_mode)


def shift1d_fixed_func(input: Tensor, shifts: Tensor, padding_mode: int, borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H] tensor by the integers of shifts [C, 1]; borders [1, 2] = (cut_left, cut_right)."""
    return _shift_fixed_func(1, input, shifts, padding_mode, borders)


def shift2d_fixed_func(input: Tensor, shifts: Tensor, padding_mode: int, borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H, W] tensor by the integers of shifts [C, 2] (H, W); borders [2, 2]."""
    return _shift_fixed_func(2, input, shifts, padding_mode, borders)


def shift3d_fixed_func(input: Tensor, shifts: Tensor, padding_mode: int, borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H, W, D] tensor by the integers of shifts [C, 3] (H, W, D); borders [3, 2]."""
    return _shift_fixed_func(3, input, shifts, padding_mode, borders)


# ---- fixed shift + average pool as one op -----------------------------------------------------------------------------------
# `pool` is the window (= stride) per spatial dim, an int or a list.  The result equals
# avg_pool{N}d(shift{N}d_fixed_func(...), kernel_size=pool, stride=pool, ceil_mode=True), the tail of a fixed layer that emulates a
# strided depthwise conv.  On HIP tensors the full-size shift output is never written (the fused sparse forward under the table) and
# the backward gathers the input gradient straight from the pooled gradient, one division per element: the autograd node keeps the
# table, the borders, the input's sizes and the pool, no tensor of the input's size.  On CPU tensors the op is that two-step sequence.
def shift1d_fixed_pool_func(input: Tensor, shifts: Tensor, padding_mode: int, pool=2, borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H] tensor by the integers of shifts [C, 1], then avg_pool1d(kernel_size=pool, stride=pool, ceil_mode=True),
    as one op; pool: an int or 1 window sizes; borders [1, 2] = (cut_left, cut_right) per dim."""
    return _shift_fixed_func(1, input, shifts, padding_mode, borders, pool)


def shift2d_fixed_pool_func(input: Tensor, shifts: Tensor, padding_mode: int, pool=2, borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H, W] tensor by the integers of shifts [C, 2] (H, W), then avg_pool2d(kernel_size=pool, stride=pool, ceil_mode=True),
    as one op; pool: an int or 2 window sizes; borders [2, 2] = (cut_left, cut_right) per dim."""
    return _shift_fixed_func(2, input, shifts, padding_mode, borders, pool)


def shift3d_fixed_pool_func(input: Tensor, shifts: Tensor, padding_mode: int, pool=2, borders: Optional[Tensor] = None) -> Tensor:
    """Shift a [N, C, H, W, D] tensor by the integers of shifts [C, 3] (H, W, D), then avg_pool3d(kernel_size=pool, stride=pool, ceil_mode=True),
    as one op; pool: an int or 3 window sizes; borders [3, 2] = (cut_left, cut_right) per dim."""
    return _shift_fixed_func(3, input, shifts, padding_mode, borders, pool)


# ---- temporal shift (TSM, arXiv 1811.08383): fixed shifts across the frames of a [N * n_segment, C, ...] tensor -----------------
# Every run of n_segment consecutive rows of dim 0 is one clip; channel c of frame t becomes channel c of frame
# pad(t - shifts[c]) of the same clip.  The result equals
#   shift2d_fixed_func(x.view(N, T, C, M).permute(0, 2, 1, 3), stack([shifts, 0], 1), padding_mode).permute(0, 2, 1, 3).reshape(x.shape)
# without either layout change: on HIP tensors one pass that copies or zero-fills whole frames' channel planes, forward and
# backward.  The autograd node keeps the table alone.  `shifts`: [n_channels] (or [n_channels, 1]) integers, or floats that hold
# integers.  Nothing validates a float table: an entry that is not an integer is rounded half to even, like the sparse shift's
# weights and the tables of shift{N}d_fixed_func.  On HIP tensors the table is converted to the input's dtype, like those tables:
# exact for |shift| <= 256 in bfloat16 and <= 2048 in float16 (clips of more frames than that in a 16-bit tensor, or larger shifts
# under periodic / reflect / symmetric padding, would be rounded; the CPU op uses the integers as they are).
#
# memory_format: torch.contiguous_format (the default) returns a contiguous result whatever the input's layout.  With
# torch.preserve_format a dense channels-last input (3 to 5 dims, unit channel stride, not contiguous: torch.channels_last,
# torch.channels_last_3d, or [N * n_segment, C, L] with strides (L * C, 1, C)) comes back in its own strides, and x.grad takes the
# layout of the incoming gradient by the same rule; every other input gives what the default gives.  On HIP tensors the
# channels-last tensor is shifted as it lies, one pass with no layout change in either direction, and its table is float32 for
# 16-bit tensors: exact for every shift.
def temporal_shift_func(input: Tensor, shifts: Tensor, n_segment: int, padding_mode: int = 0,
                        memory_format: torch.memory_format = torch.contiguous_format) -> Tensor:
    """Shift the channels of a [N * n_segment, C, ...] tensor (2 to 5 dims) across the n_segment frames of each clip."""
    name = "temporal_shift_func()"
    _assert_has_ops()
    assert memory_format in (torch.contiguous_format, torch.preserve_format), \
        f"{name} expected memory_format to be torch.contiguous_format or torch.preserve_format, but it is {memory_format}"
    assert padding_mode in [0, 1, 2, 3, 4], f"{name} expected padding_mode can be {_PADDING_DOC}"
    assert 2 <= len(input.shape) <= 5, f"{name}: expected a 2D to 5D tensor as input, but it is shape is {input.shape}"
    assert isinstance(n_segment, int) and n_segment >= 1 and input.shape[0] % n_segment == 0, \
        f"{name}: expected dim 0 of the input ({input.shape[0]}) to be a multiple of n_segment ({n_segment})"
    assert len(shifts.shape) == 1 or (len(shifts.shape) == 2 and shifts.shape[1] == 1), \
        f"{name}: expected [n_channels] tensor as shifts, but it is shape is {shifts.shape}"
    assert input.shape[1] == shifts.shape[0], \
        (f"{name}: expected that input and shifts have equal number of channels, but input have "
         f"{input.shape[1]} and shifts have {shifts.shape[0]} channels.")
    assert input.device == shifts.device, \
        (f"{name}: expected input and shifts to be on same device, but input is  on {input.device} "
         f"and shifts is on {shifts.device}")
    if memory_format == torch.preserve_format:
        return torch.ops.torchshifts.temporal_shift_cl(input, shifts, n_segment, padding_mode)
    return torch.ops.torchshifts.temporal_shift(input, shifts, n_segment, padding_mode)


# ---- in-place temporal shift ----------------------------------------------------------------------------------------------------
# temporal_shift_func written into `input`, which is returned (the layout is the input's own, so there is no memory_format).  On
# HIP tensors a dense input -- contiguous, or dense channels-last as above -- with n_segment <= 16 is one pass over the SHIFTED
# channels alone: the kernel neither reads nor writes a channel whose shift is 0, and nothing of the input's size is allocated.  Its
# table is float32 for 16-bit tensors (exact for every shift) and the input's dtype otherwise.  Every other input (a slice, a
# non-dense view, more than 16 frames per clip) and every CPU tensor is input.copy_(temporal_shift_func(input, ...)).  Autograd: the
# input is marked dirty (a leaf that requires grad raises PyTorch's own error), the node keeps the table alone, and the backward is
# the out-of-place one of temporal_shift_func, in the layout of the input.
def temporal_shift_func_(input: Tensor, shifts: Tensor, n_segment: int, padding_mode: int = 0) -> Tensor:
    """Shift the channels of a [N * n_segment, C, ...] tensor (2 to 5 dims) across the n_segment frames of each clip, in place."""
    name = "temporal_shift_func_()"
    _assert_has_ops()
    assert padding_mode in [0, 1, 2, 3, 4], f"{name} expected padding_mode can be {_PADDING_DOC}"
    assert 2 <= len(input.shape) <= 5, f"{name}: expected a 2D to 5D tensor as input, but it is shape is {input.shape}"
    assert isinstance(n_segment, int) and n_segment >= 1 and input.shape[0] % n_segment == 0, \
        f"{name}: expected dim 0 of the input ({input.shape[0]}) to be a multiple of n_segment ({n_segment})"
    assert len(shifts.shape) == 1 or (len(shifts.shape) == 2 and shifts.shape[1] == 1), \
        f"{name}: expected [n_channels] tensor as shifts, but it is shape is {shifts.shape}"
    assert input.shape[1] == shifts.shape[0], \
        (f"{name}: expected that input and shifts have equal number of channels, but input have "
         f"{input.shape[1]} and shifts have {shifts.shape[0]} channels.")
    assert input.device == shifts.device, \
        (f"{name}: expected input and shifts to be on same device, but input is  on {input.device} "
         f"and shifts is on {shifts.device}")
    return torch.ops.torchshifts_inplace.temporal_shift_(input, shifts, n_segment, padding_mode)


# ---- learnable temporal shift: a TRAINED per-channel shift across the frames of a [N * n_segment, C, ...] tensor -----------------
# The sparse (rounded) or active (interpolated) 1-D shift of shift1d_func, applied along the frames of each clip.  The result, and
# the gradients of input and weights, equal those of
#   shift1d_func(x.view(N, T, C, M).permute(0, 3, 2, 1).reshape(N * M, C, T), weights.view(C, 1), padding_mode, active_flag)
#       .view(N, M, C, T).permute(0, 3, 2, 1).reshape(x.shape)
# without either layout change and without a permuted copy of the input in the autograd node: on HIP tensors one kernel per pass.
# (The [N, C, T, M] view through shift2d_func with weights (w, 0) is NOT the same thing: the 2-D rule wires a difference along the
# second dim into the first dim's weight gradient.)  `weights`: [n_channels] or [n_channels, 1] floats of the input's dtype, or
# float32 with a float16 / bfloat16 input (torch.autocast); weights.grad has the weights' dtype.
#
# memory_format: torch.contiguous_format (the default) is the call above, a contiguous result whatever the input's layout.  With
# torch.preserve_format a dense channels-last input (as for temporal_shift_func) comes back in its own strides with the same
# values, and x.grad takes the layout of the incoming gradient when that is dense channels-last too; every other input gives what
# the default gives.  On HIP tensors the channels-last tensors are served as they lie, one kernel per pass, no layout change in
# either direction, and the autograd node keeps the input without a copy.
def temporal_shift_learnable_func(input: Tensor, weights: Tensor, n_segment: int, padding_mode: int = 0,
                                  active_flag: bool = False,
                                  memory_format: torch.memory_format = torch.contiguous_format) -> Tensor:
    """Shift the channels of a [N * n_segment, C, ...] tensor (2 to 5 dims) across the n_segment frames of each clip by weights[c]."""
    name = "temporal_shift_learnable_func()"
    _assert_has_ops()
    assert memory_format in (torch.contiguous_format, torch.preserve_format), \
        f"{name} expected memory_format to be torch.contiguous_format or torch.preserve_format, but it is {memory_format}"
    assert padding_mode in [0, 1, 2, 3, 4], f"{name} expected padding_mode can be {_PADDING_DOC}"
    assert 2 <= len(input.shape) <= 5, f"{name}: expected a 2D to 5D tensor as input, but it is shape is {input.shape}"
    assert isinstance(n_segment, int) and n_segment >= 1 and input.shape[0] % n_segment == 0, \
        f"{name}: expected dim 0 of the input ({input.shape[0]}) to be a multiple of n_segment ({n_segment})"
    assert len(weights.shape) == 1 or (len(weights.shape) == 2 and weights.shape[1] == 1), \
        f"{name}: expected [n_channels] or [n_channels,1] tensor as weight, but it is shape is {weights.shape}"
    assert input.shape[1] == weights.shape[0], \
        (f"{name}: expected that input and weight have equal number of channels, but input have "
         f"{input.shape[1]} and weight have {weights.shape[0]} channels.")
    assert weights.is_floating_point(), f"{name}: expected float weights, but they are {weights.dtype}"
    assert input.device == weights.device, \
        (f"{name}: expected input and weights to be on same device, but input is  on {input.device} "
         f"and weights is on {weights.device}")
    if memory_format == torch.preserve_format:
        return torch.ops.torchshifts.temporal_shift_learnable_cl(input, weights, n_segment, padding_mode, bool(active_flag))
    return torch.ops.torchshifts.temporal_shift_learnable(input, weights, n_segment, padding_mode, bool(active_flag))


# ---- per-clip temporal shift: a table of shape [N, n_channels], one row per clip of a [N * n_segment, C, ...] tensor ------------------
# The temporal shifts above under a table that differs from clip to clip -- a shift that a small net predicts from the clip itself
# (the Temporal Interlacing Network's OffsetNet, arXiv 2001.06499), or per-clip temporal jitter.  By definition, for every clip n,
#   out[n*T:(n+1)*T] = temporal_shift_learnable_func(x[n*T:(n+1)*T], weights[n], T, padding_mode, active_flag)
# (temporal_shift_func for the fixed form), with that call's x.grad, and weights.grad[n] that call's weights.grad, in both modes.
# On HIP tensors it is ONE kernel per pass, the kernel of temporal_shift_learnable_func, instead of N launches and a cat: out and
# x.grad carry the loop's bits, weights.grad is deterministic.  The result is contiguous.
# The table is [N, n_channels], or [N, n_groups] with n_channels % n_groups == 0 (TIN's groups: entry g serves the n_channels //
# n_groups consecutive channels of group g); a group table is expanded here, so autograd sums a group's gradient.
#
# memory_format: torch.contiguous_format (the default) is the call above.  With torch.preserve_format a dense channels-last input (as
# for temporal_shift_func) comes back in its own strides with the same values, and x.grad takes the layout of the incoming gradient
# when that is dense channels-last too; every other input gives what the default gives.  On HIP tensors the channels-last tensors
# are served as they lie, one kernel per pass (the frame kernels under the clip's row of the table), no layout change in either
# direction.  A group table whose groups are whole 16-byte pieces of a pixel's channel row takes those kernels' fast path.
def _per_clip_table(name: str, input: Tensor, table: Tensor, n_segment: int, padding_mode: int, kind: str) -> Tensor:
    _assert_has_ops()
    assert padding_mode in [0, 1, 2, 3, 4], f"{name} expected padding_mode can be {_PADDING_DOC}"
    assert 2 <= len(input.shape) <= 5, f"{name}: expected a 2D to 5D tensor as input, but it is shape is {input.shape}"
    assert isinstance(n_segment, int) and n_segment >= 1 and input.shape[0] % n_segment == 0, \
        f"{name}: expected dim 0 of the input ({input.shape[0]}) to be a multiple of n_segment ({n_segment})"
    assert not input.is_quantized, f"{name}: quantized inputs are not supported"
    clips, channels = input.shape[0] // n_segment, input.shape[1]
    assert (len(table.shape) == 2 and table.shape[0] == clips and table.shape[1] >= 1 and channels % table.shape[1] == 0), \
        (f"{name}: expected [{clips}, {channels}] tensor (one row per clip; or [{clips}, n_groups] with {channels} % n_groups == 0) "
         f"as {kind}, but it is shape is {table.shape}")
    assert input.device == table.device, \
        (f"{name}: expected input and {kind} to be on same device, but input is  on {input.device} "
         f"and {kind} is on {table.device}")
    if table.shape[1] != channels:
        table = table.repeat_interleave(channels // table.shape[1], dim=1)
    return table


def temporal_shift_per_clip_func(input: Tensor, shifts: Tensor, n_segment: int, padding_mode: int = 0,
                                 memory_format: torch.memory_format = torch.contiguous_format) -> Tensor:
    """Shift the channels of a [N * n_segment, C, ...] tensor (2 to 5 dims) across the frames of each clip by the integers
    shifts[n, c] of its own clip n.  Floats are rounded half to even; the autograd node keeps the table alone.
    memory_format=torch.preserve_format keeps a dense channels-last input's layout.  On the GPU it pays under a GROUP table whose
    groups span whole 16-byte pieces of a pixel's channel row (8 fp16 / 4 fp32 channels or more); under an ungrouped [N, C] table
    keep the default: the backward then moves channels one by one and is slower than the default route with its layout changes."""
    name = "temporal_shift_per_clip_func()"
    assert memory_format in (torch.contiguous_format, torch.preserve_format), \
        f"{name} expected memory_format to be torch.contiguous_format or torch.preserve_format, but it is {memory_format}"
    shifts = _per_clip_table(name, input, shifts, n_segment, padding_mode, "shifts")
    if memory_format == torch.preserve_format:
        return torch.ops.torchshifts_per_clip_cl.temporal_shift_per_clip_cl(input, shifts, n_segment, padding_mode)
    return torch.ops.torchshifts_per_clip.temporal_shift_per_clip(input, shifts, n_segment, padding_mode)


def temporal_shift_learnable_per_clip_func(input: Tensor, weights: Tensor, n_segment: int, padding_mode: int = 0,
                                           active_flag: bool = False,
                                           memory_format: torch.memory_format = torch.contiguous_format) -> Tensor:
    """Shift the channels of a [N * n_segment, C, ...] tensor (2 to 5 dims) across the frames of each clip by weights[n, c] of its
    own clip n, sparse (rounded) or active (interpolated); differentiable in input and weights."""
    name = "temporal_shift_learnable_per_clip_func()"
    assert memory_format in (torch.contiguous_format, torch.preserve_format), \
        f"{name} expected memory_format to be torch.contiguous_format or torch.preserve_format, but it is {memory_format}"
    assert weights.is_floating_point(), f"{name}: expected float weights, but they are {weights.dtype}"
    weights = _per_clip_table(name, input, weights, n_segment, padding_mode, "weights")
    if memory_format == torch.preserve_format:
        return torch.ops.torchshifts_per_clip_cl.temporal_shift_learnable_per_clip_cl(input, weights, n_segment, padding_mode,
                                                                                      bool(active_flag))
    return torch.ops.torchshifts_per_clip.temporal_shift_learnable_per_clip(input, weights, n_segment, padding_mode, bool(active_flag))


# ---- temporal interlacing (the TIN layer, arXiv 2001.06499): the per-clip shift fused with a per-clip, per-frame weight --------------
# By definition, with N = input.shape[0] // n_segment, offsets [N, C] and scales [N, T, C]:
#   y   = temporal_shift_learnable_per_clip_func(input, offsets, n_segment, padding_mode, active_flag)
#   out = y * scales.reshape(N * T, C, 1, ...)                # out[n, t, c, :] = scales[n, t, c] * shift(x)[n, t, c, :]
# and the gradients are that composition's: input.grad is the per-clip backward of scales * grad_out, offsets.grad its table gradient,
# scales.grad[n, t, c] the sum over the plane of grad_out * y.  CPU tensors run exactly that.  On HIP tensors each pass is ONE kernel
# (csrc/shiftnd_interlace.hip): the forward reads and writes the tensor once, the backward has the traffic of the per-clip backward
# alone, and the autograd node keeps input, offsets and scales -- no shifted activation of the output's size.  float32 / float64 out
# and input.grad carry the composition's bits; float16 / bfloat16 are interpolated and scaled in float32 and rounded once; both table
# gradients are deterministic.  Group tables [N, G] / [N, T, G] (C % G == 0) are expanded here, so autograd sums a group's gradient.
#
# memory_format: torch.contiguous_format (the default) is the call above, a contiguous result whatever the input's layout.  With
# torch.preserve_format a dense channels-last input (as for temporal_shift_func) comes back in its own strides with the same values,
# and input.grad takes the layout of the incoming gradient when that is dense channels-last too; every other input gives what the
# default gives.  On HIP tensors the channels-last tensors are served as they lie, one kernel per pass
# (csrc/shiftnd_interlace_frames.hip), no layout change in either direction, any n_segment; the node keeps input, offsets and scales.
# The TIN layer's own tables (four channel groups over the fold) make every 16-byte piece of a pixel's channel row uniform, the
# kernels' fast path; an ungrouped [N, C] table moves channels one by one.
def temporal_interlace_func(input: Tensor, offsets: Tensor, scales: Tensor, n_segment: int, padding_mode: int = 0,
                            active_flag: bool = True, memory_format: torch.memory_format = torch.contiguous_format) -> Tensor:
    """Shift the channels of a [N * n_segment, C, ...] tensor (2 to 5 dims) across the frames of each clip by offsets[n, c]
    (out[t] = x[t - w]; interpolated with active_flag, rounded without) and weight frame t of clip n by scales[n, t, c];
    differentiable in input, offsets and scales.  offsets: [N, C] or [N, G]; scales: [N, n_segment, C] or [N, n_segment, G].
    memory_format=torch.preserve_format keeps a dense channels-last input's layout; such a call needs N * n_segment * C < 2^31 (the
    packed table's index, as the default call does) and raises a RuntimeError ("invalid argument") beyond it.  On the GPU it pays
    in the forward and in memory; for float16 / bfloat16 TRAINING the composition temporal_shift_learnable_per_clip_func(...,
    memory_format=torch.preserve_format) * scales is currently faster (README)."""
    name = "temporal_interlace_func()"
    assert memory_format in (torch.contiguous_format, torch.preserve_format), \
        f"{name} expected memory_format to be torch.contiguous_format or torch.preserve_format, but it is {memory_format}"
    assert offsets.is_floating_point(), f"{name}: expected float offsets, but they are {offsets.dtype}"
    assert scales.is_floating_point(), f"{name}: expected float scales, but they are {scales.dtype}"
    offsets = _per_clip_table(name, input, offsets, n_segment, padding_mode, "offsets")
    clips, channels = input.shape[0] // n_segment, input.shape[1]
    assert (len(scales.shape) == 3 and scales.shape[0] == clips and scales.shape[1] == n_segment and scales.shape[2] >= 1
            and channels % scales.shape[2] == 0), \
        (f"{name}: expected [{clips}, {n_segment}, {channels}] tensor (one entry per clip, frame and channel; or [{clips}, {n_segment}, "
         f"n_groups] with {channels} % n_groups == 0) as scales, but it is shape is {scales.shape}")
    assert input.device == scales.device, \
        (f"{name}: expected input and scales to be on same device, but input is  on {input.device} "
         f"and scales is on {scales.device}")
    assert scales.dtype == offsets.dtype, f"{name}: expected offsets and scales of one dtype, but they are {offsets.dtype} and {scales.dtype}"
    if scales.shape[2] != channels:
        scales = scales.repeat_interleave(channels // scales.shape[2], dim=2)
    if memory_format == torch.preserve_format:
        return torch.ops.torchshifts_interlace_cl.temporal_interlace_cl(input, offsets, scales, n_segment, padding_mode, bool(active_flag))
    return torch.ops.torchshifts_interlace.temporal_interlace(input, offsets, scales, n_segment, padding_mode, bool(active_flag))


# ---- online temporal shift: one frame per call against a cached state (the uni-directional TSM, arXiv 1811.08383 section 4.2) ------
# Frames of B independent streams arrive one at a time as [B, C, ...]; the channels that shift are taken from a state of the previous
# frames.  Sign convention of temporal_shift_func: out[t] = x[t - shifts[c]], so an online table is CAUSAL, every entry >= 0, and the
# state has D = max(shifts) slots of the frame's shape and layout, state[k] holding frame t-1-k.  One step, for every channel c with
# s = shifts[c] > 0:
#   out[:, c] = state[s-1][:, c];   state[k][:, c] = state[k-1][:, c] for k = s-1 .. 1;   state[0][:, c] = x[:, c]
# Channels with shift 0 are neither read nor written, in the frame or in the state.  Feeding the T frames of a clip-major
# [B * T, C, ...] tensor one at a time gives, stacked, temporal_shift_func(X, shifts, T, padding_mode) bit for bit: a state of zeros
# (the zero point of a quantized tensor) is padding_mode 0, a state whose every slot holds the first frame is padding_mode 1
# (border).  Periodic, reflect and symmetric padding look into the future and are refused.
# On HIP tensors a dense frame (contiguous, or dense channels-last as for temporal_shift_func) with D <= 15 is ONE kernel over the
# shifted channels alone -- under the default table an eighth of the frame -- with no host synchronisation, so a step can be captured
# in a torch.cuda.graph; with a table of the kernel's kind (float32 for 16-bit tensors, the tensor's dtype for float32 / float64,
# int32 for quantized tensors; OnlineTemporalShift keeps one) nothing is allocated either, any other table is converted per call.
# Every other input (CPU tensors, D > 15, views that are not dense) runs a composite of index_select / index_copy_ with the same
# values; the composite reads the table on the host.  Inference only: a tensor that requires grad raises.
def _online_checks(name: str, input: Tensor, shifts: Tensor):
    _assert_has_ops()
    assert 2 <= len(input.shape) <= 5, f"{name}: expected a 2D to 5D tensor [B, C, ...] as input, but it is shape is {input.shape}"
    assert len(shifts.shape) == 1 and input.shape[1] == shifts.shape[0], \
        f"{name}: expected [{input.shape[1]}] tensor as shifts, but it is shape is {shifts.shape}"
    assert input.device == shifts.device, \
        (f"{name}: expected input and shifts to be on same device, but input is  on {input.device} "
         f"and shifts is on {shifts.device}")


def temporal_shift_online_table(input: Tensor, shifts: Tensor) -> Tensor:
    """`shifts` in the kind the HIP kernel reads for `input`: a step given this table allocates nothing."""
    if input.is_quantized:
        kind = torch.int32
    else:
        kind = torch.float32 if input.dtype in (torch.float16, torch.bfloat16) else input.dtype
    s = shifts.detach()
    if kind == torch.int32 and s.is_floating_point():
        s = torch.round(s)
    return s.to(kind).contiguous()


def temporal_shift_online_state(input: Tensor, shifts: Tensor, padding_mode: int = 0) -> Tensor:
    """The initial state [D, B, C, ...] for frames like `input` under the causal table `shifts`, D = max(shifts), in the input's
    layout: zeros (the zero point) for padding_mode 0, the input's own values in every slot for padding_mode 1 (pass the FIRST
    frame).  Validates the table -- integers, all >= 0 -- with the one host synchronisation of the feature."""
    name = "temporal_shift_online_state()"
    _online_checks(name, input, shifts)
    if padding_mode not in (0, 1):
        raise ValueError(f"{name}: padding_mode must be 0 (zeros) or 1 (border); periodic, reflect and symmetric padding look into "
                         f"the future, and it is {padding_mode}")
    s = shifts.detach()
    if s.is_floating_point():
        if not bool((s == torch.round(s)).all()):
            raise ValueError(f"{name}: shifts must hold integers")
    elif s.dtype == torch.bool or s.is_complex():
        raise ValueError(f"{name}: shifts must hold integers")
    low, high = (int(s.min()), int(s.max())) if s.numel() else (0, 0)
    if low < 0:
        raise ValueError(f"{name}: a negative shift ({low}) reads the future; an online table is causal (every entry >= 0)")
    # the buffer in memory order, a view of it in the input's layout (contiguous, or dense channels-last in every slot, the slots one
    # frame batch apart); a quantized state wraps the same bytes (the wrapper makes a contiguous copy, so the view is taken last)
    shape = (high,) + tuple(input.shape)
    plain = input.int_repr() if input.is_quantized else input.detach()
    memory = torch.empty(shape, dtype=plain.dtype, device=plain.device)

    def lay(t):
        dense = input.numel() > 0 and (input.is_contiguous() or _is_channels_last_dense(input))
        return t.as_strided(shape, (input.numel(),) + tuple(input.stride())) if high and dense else t

    if padding_mode == 1:
        lay(memory).copy_(plain.unsqueeze(0).expand(shape))
    else:
        memory.fill_(input.q_zero_point() if input.is_quantized else 0)
    if input.is_quantized:
        memory = torch._make_per_tensor_quantized_tensor(memory, input.q_scale(), input.q_zero_point())
    return lay(memory)


def _is_channels_last_dense(t: Tensor) -> bool:
    if t.dim() < 3 or t.numel() == 0 or t.shape[1] < 2 or t.is_contiguous() or t.stride(1) != 1:
        return False
    expect = t.shape[1]
    for d in range(t.dim() - 1, 1, -1):
        if t.shape[d] != 1 and t.stride(d) != expect:
            return False
        expect *= t.shape[d]
    return t.shape[0] == 1 or t.stride(0) == expect


def temporal_shift_online_func_(input: Tensor, state: Tensor, shifts: Tensor) -> Tensor:
    """One online step in place on both tensors: `input` [B, C, ...] becomes the shifted frame and is returned, `state`
    [D, B, C, ...] (temporal_shift_online_state) takes the incoming frame's shifted channels."""
    name = "temporal_shift_online_func_()"
    _online_checks(name, input, shifts)
    assert not input.is_quantized, f"{name}: quantized inputs go through torchshifts.quantized.functional.temporal_shift_online_quantized_"
    return torch.ops.torchshifts_online.temporal_shift_online_(input, state, shifts)


def temporal_shift_online_func(input: Tensor, state: Tensor, shifts: Tensor) -> Tensor:
    """temporal_shift_online_func_ on input.clone(): the input is left as it was, the state is still updated."""
    return temporal_shift_online_func_(input.clone(memory_format=torch.preserve_format), state, shifts)
