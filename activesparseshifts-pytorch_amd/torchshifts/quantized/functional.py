"""Quantized functional wrappers (reference torchshifts/quantized/functional.py:3-15)."""
import torch

from torchshifts.extension import _assert_has_ops
from torchshifts.functional import shift1d_func, shift2d_func, shift3d_func


def _quantized(name, func, input, weight, padding_mode, cut_borders):
    if not input.is_quantized:
        raise ValueError(f"Input to '{name}' must be quantized!")
    return func(input, weight, padding_mode, False, cut_borders)


def shift1d_quantized(input, weight, padding_mode, cut_borders=None):
    return _quantized('shift1d_quantized', shift1d_func, input, weight, padding_mode, cut_borders)


def shift2d_quantized(input, weight, padding_mode, cut_borders=None):
    return _quantized('shift2d_quantized', shift2d_func, input, weight, padding_mode, cut_borders)


def shift3d_quantized(input, weight, padding_mode, cut_borders=None):
    return _quantized('shift3d_quantized', shift3d_func, input, weight, padding_mode, cut_borders)


def temporal_shift_quantized(input, shifts, n_segment, padding_mode=0, memory_format=torch.contiguous_format):
    """The temporal shift (torchshifts.functional.temporal_shift_func) of a per-tensor quantized [N * n_segment, C, ...] tensor
    (quint8, qint8, qint32; 2 to 5 dims): the same gather on the int_repr, with the input's zero point where zeros padding fills
    (it dequantizes to exactly 0).  Scale and zero point are the input's -- nothing is requantized -- and the result is
    contiguous.  `shifts`: [n_channels] or [n_channels, 1] integers, or floats rounded half to even.  On HIP tensors the table
    is converted to int32, exact for every shift (the float op's table has the tensor's 16-bit dtype).  No gradient.
    memory_format=torch.preserve_format: a dense channels-last input comes back in its own strides (on HIP tensors shifted as it
    lies, one pass); every other input, and the default torch.contiguous_format, give the contiguous result."""
    if not input.is_quantized:
        raise ValueError("Input to 'temporal_shift_quantized' must be quantized!")
    _assert_has_ops()
    assert memory_format in (torch.contiguous_format, torch.preserve_format), \
        f"temporal_shift_quantized expected memory_format to be torch.contiguous_format or torch.preserve_format, but it is {memory_format}"
    if memory_format == torch.preserve_format:
        return torch.ops.torchshifts.temporal_shift_quantized_cl(input, shifts, int(n_segment), int(padding_mode))
    return torch.ops.torchshifts.temporal_shift_quantized(input, shifts, int(n_segment), int(padding_mode))


def temporal_shift_learnable_quantized(input, weights, n_segment, padding_mode=0, active_flag=True,
                                       memory_format=torch.contiguous_format):
    """The learnable temporal shift (torchshifts.functional.temporal_shift_learnable_func) of a per-tensor quantized
    [N * n_segment, C, ...] tensor (quint8, qint8, qint32; 2 to 5 dims) under a trained fp32 table `weights` ([n_channels] or
    [n_channels, 1], not requiring grad).  The result is defined in the integer domain: with q = input.int_repr(), zp the zero point
    and F = fp32 (8-bit types) or fp64 (qint32),

        out = clamp(zp + rint(temporal_shift_learnable_func((q - zp).to(F), weights.to(F), n_segment, padding_mode, True)))

    rint half to even; zeros padding contributes 0, which is the zero point in the result.  The scale does not enter, nothing is
    dequantized or requantized: the result has the input's scale, zero point and dtype, and is contiguous (a channels-last input
    is made contiguous first).  On HIP tensors it is one kernel with the table passed as it is.  active_flag=False is
    temporal_shift_quantized(input, weights, n_segment, padding_mode): the table rounded half to even.  No gradient.
    memory_format=torch.preserve_format: a dense channels-last input (torch.channels_last, torch.channels_last_3d, or
    [N * n_segment, C, L] with unit channel stride) comes back in its own strides with the same values, bit for bit -- on HIP
    tensors interpolated as it lies, one kernel, nothing allocated but the output; active_flag=False is then
    temporal_shift_quantized(..., memory_format=torch.preserve_format).  Every other input, and the default
    torch.contiguous_format, give the contiguous result."""
    if not input.is_quantized:
        raise ValueError("Input to 'temporal_shift_learnable_quantized' must be quantized!")
    _assert_has_ops()
    assert memory_format in (torch.contiguous_format, torch.preserve_format), \
        f"temporal_shift_learnable_quantized expected memory_format to be torch.contiguous_format or torch.preserve_format, but it is {memory_format}"
    if memory_format == torch.preserve_format:
        return torch.ops.torchshifts_quantized_learnable_cl.temporal_shift_learnable_quantized_cl(input, weights, int(n_segment),
                                                                                                  int(padding_mode), bool(active_flag))
    return torch.ops.torchshifts_quantized_learnable.temporal_shift_learnable_quantized(input, weights, int(n_segment), int(padding_mode),
                                                                                         bool(active_flag))


def _expand_groups(table, channels):
    """a group table [..., G] (C % G == 0) as [..., C], entry g serving the C // G consecutive channels of group g; every other
    table as it is (the op names what is wrong with it)"""
    groups = table.shape[-1] if table.dim() >= 2 else 0
    if groups >= 1 and groups != channels and channels % groups == 0:
        return table.repeat_interleave(channels // groups, dim=table.dim() - 1)
    return table


def temporal_interlace_quantized(input, offsets, scales, n_segment, padding_mode=0, active_flag=True):
    """Temporal interlacing (torchshifts.functional.temporal_interlace_func, the TIN layer's core) of a per-tensor quantized
    [N * n_segment, C, ...] tensor (quint8, qint8, qint32; 2 to 5 dims) under fp32 tables that do not require grad: offsets [N, C]
    (or [N, G], C % G == 0) and scales [N, n_segment, C] (or [N, n_segment, G]); scales=None is the per-clip shift alone, equal to
    scales of ones.  The result is defined in the integer domain: with q = input.int_repr(), zp the zero point and F = fp32 (8-bit
    types) or fp64 (qint32),

        out = clamp(zp + rint(temporal_interlace_func((q - zp).to(F), offsets.to(F), scales.to(F), n_segment, padding_mode, active_flag)))

    rint half to even; the interpolation is the float op's (two multiplies, one add), then ONE multiply by the plane's scale; zeros
    padding contributes 0, which is the zero point in the result under any finite scale.  The tensor's scale does not enter, nothing
    is dequantized or requantized: the result has the input's scale, zero point and dtype, and is contiguous (a channels-last input
    is made contiguous first).  A scale entry above 1 can therefore SATURATE -- the clamp to the dtype's range is part of the
    definition; TIN's WeightNet yields weights in (0, 2), so choose the activation's quantization range with that headroom.
    active_flag=False rounds the offsets half to even and still applies the scales.  Offsets and scales must be finite (not
    validated: no host synchronisation).  On HIP tensors it is one kernel.  No gradient."""
    if not input.is_quantized:
        raise ValueError("Input to 'temporal_interlace_quantized' must be quantized!")
    _assert_has_ops()
    channels = input.shape[1] if input.dim() >= 2 else 0
    offsets = _expand_groups(offsets, channels)
    if scales is not None:
        scales = _expand_groups(scales, channels)
    return torch.ops.torchshifts_quantized_interlace.temporal_interlace_quantized(input, offsets, scales, int(n_segment), int(padding_mode),
                                                                                  bool(active_flag))


def temporal_shift_learnable_per_clip_quantized(input, weights, n_segment, padding_mode=0, active_flag=True):
    """The per-clip temporal shift (torchshifts.functional.temporal_shift_learnable_per_clip_func) of a per-tensor quantized
    [N * n_segment, C, ...] tensor under an fp32 table `weights` [N, C] (or [N, G], C % G == 0), one row per clip:
    temporal_interlace_quantized without scales -- the same integer-domain definition, the same kernel, nothing saturates.
    active_flag=False rounds the table half to even (the fixed per-clip shift, PerClipTemporalShift).  No gradient."""
    if not input.is_quantized:
        raise ValueError("Input to 'temporal_shift_learnable_per_clip_quantized' must be quantized!")
    return temporal_interlace_quantized(input, weights, None, n_segment, padding_mode, active_flag)


def temporal_shift_quantized_(input, shifts, n_segment, padding_mode=0):
    """temporal_shift_quantized written into `input`, which is returned with its scale, zero point and layout (the in-place
    torchshifts.functional.temporal_shift_func_ of a per-tensor quantized tensor).  On HIP tensors a dense input -- contiguous or
    dense channels-last -- with n_segment <= 16 is one pass over the shifted channels alone, with an int32 table and nothing of
    the input's size allocated; every other input, and every CPU tensor, is the out-of-place result copied into the input."""
    if not input.is_quantized:
        raise ValueError("Input to 'temporal_shift_quantized_' must be quantized!")
    _assert_has_ops()
    return torch.ops.torchshifts_inplace.temporal_shift_quantized_(input, shifts, int(n_segment), int(padding_mode))


def temporal_shift_online_quantized_(input, state, shifts):
    """One online step (torchshifts.functional.temporal_shift_online_func_) on a per-tensor quantized frame [B, C, ...] (quint8,
    qint8, qint32) and its quantized state [D, B, C, ...] (temporal_shift_online_state: the input's scale and zero point, the zero
    point in every slot for zeros padding; any other state raises).  Both are written, `input` is returned with its scale, zero
    point and layout.  On HIP tensors a dense frame with D <= 15 is one kernel over the shifted channels alone, with an int32 table."""
    if not input.is_quantized:
        raise ValueError("Input to 'temporal_shift_online_quantized_' must be quantized!")
    _assert_has_ops()
    return torch.ops.torchshifts_online.temporal_shift_online_quantized_(input, state, shifts)


def temporal_shift_online_quantized(input, state, shifts):
    """temporal_shift_online_quantized_ on a clone of `input`: the input is left as it was, the state is still updated."""
    if not input.is_quantized:
        raise ValueError("Input to 'temporal_shift_online_quantized' must be quantized!")
    return temporal_shift_online_quantized_(input.clone(memory_format=torch.preserve_format), state, shifts)
