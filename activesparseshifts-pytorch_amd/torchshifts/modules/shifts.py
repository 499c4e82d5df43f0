"""Shift1d / Shift2d / Shift3d modules (surface of the reference's torchshifts/modules/shifts.py).

Constructor arguments, attribute names (`weight`, `padding`, `cut_borders`, `init_shift`,
`sparsity_term`, ...), the `(output, loss)` return convention and the depthwise-conv emulation
heuristics follow the reference so that checkpoints and calling code carry over unchanged.
Behavioural quirks of the reference that user code may depend on are kept and marked `QUIRK`.
"""
import random
from functools import partial

import torch
from torch import nn

from torchshifts.functional import (shift1d_fixed_func, shift1d_fixed_pool_func, shift1d_func, shift1d_pool_func, shift2d_fixed_func,
                                    shift2d_fixed_pool_func, shift2d_func, shift2d_pool_func, shift3d_fixed_func,
                                    shift3d_fixed_pool_func, shift3d_func, shift3d_pool_func, temporal_shift_func, temporal_shift_func_,
                                    temporal_interlace_func, temporal_shift_learnable_func, temporal_shift_learnable_per_clip_func,
                                    temporal_shift_online_func, temporal_shift_online_func_, temporal_shift_online_state,
                                    temporal_shift_online_table, temporal_shift_per_clip_func)

paddings_dict = {'zeros': 0, 'border': 1, 'periodic': 2, 'reflect': 3, 'symmetric': 4}

_SHIFT_FUNCS = {1: shift1d_func, 2: shift2d_func, 3: shift3d_func}
_SHIFT_POOL_FUNCS = {1: shift1d_pool_func, 2: shift2d_pool_func, 3: shift3d_pool_func}
_SHIFT_FIXED_FUNCS = {1: shift1d_fixed_func, 2: shift2d_fixed_func, 3: shift3d_fixed_func}
_SHIFT_FIXED_POOL_FUNCS = {1: shift1d_fixed_pool_func, 2: shift2d_fixed_pool_func, 3: shift3d_fixed_pool_func}
_AVG_POOLS = {1: torch.nn.functional.avg_pool1d, 2: torch.nn.functional.avg_pool2d, 3: torch.nn.functional.avg_pool3d}


def _wrap_dim(val, dim, name):
    """scalar / tuple / list -> list of length `dim` (reference modules/shifts.py:10-18)."""
    if isinstance(val, tuple):
        val = list(val)
    if not isinstance(val, list):
        val = [val] * dim
    if len(val) != dim:
        print(f'{name} params has different kernel sizes, but length of list do not corresponds to dim: {dim}, '
              'and was reduced')
        val = val[:dim]
    return val


def _create_dw_emulation(args, dim):
    """Heuristics that make a shift layer mimic a depthwise conv (reference modules/shifts.py:21-57).

    Returns (init_shift, scales, borders, padding):
      borders  [dim, 2] long tensor of (cut_left, cut_right) when 2*padding - kernel_size + 1 < 0
               (the conv would shrink the output), else None
      init_shift = kernel_size // (2 if init_thumb_rule_type == 1 else 1)
      scales   = stride as a [1, dim] tensor (used both as a weight scale and as the avg-pool size)
      padding  = conv padding_mode translated to the shift numbering, or -1
    """
    assert isinstance(args, dict), 'args must be dict'
    assert 'kernel_size' in args, 'args must contains at least the kernel_size inside'
    if 'dilation' in args:
        print('Warning! Found the dilation param which is not supported and will be ignored')
    kernel_size = torch.tensor(_wrap_dim(args['kernel_size'], dim, 'kernel_size'), requires_grad=False)
    padding = torch.tensor(_wrap_dim(args.get('padding', 0), dim, 'padding'), requires_grad=False)
    stride = _wrap_dim(args.get('stride', 1), dim, 'stride')
    itrt_scale = 2 if args['init_thumb_rule_type'] == 1 else 1

    borders = None
    shrink = 2 * padding - kernel_size + 1
    if (shrink < 0).any():
        borders = torch.zeros(dim, 2, dtype=torch.long, requires_grad=False)
        neg = shrink < 0
        borders[neg, 0] = abs(shrink[neg]) // 2
        borders[neg, 1] = abs(shrink[neg]) - borders[neg, 0]

    init_shift = kernel_size // itrt_scale
    scales = torch.tensor(stride, requires_grad=False).unsqueeze(0)

    pad_conv = {'zeros': 0, 'replicate': 1, 'circular': 2, 'reflect': 3}
    pad_mode = args.get('padding_mode', -1)
    if isinstance(pad_mode, str):
        pad_mode = pad_conv[pad_mode]
    return init_shift, scales, borders, pad_mode


class _Shiftnd(nn.Module):
    """Base of all shift modules.

    Arguments:
        in_channels (int): channels of the input.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        init_shift (float / tuple): bound of the uniform weight initialisation. Default 1.
        sparsity_term (float): strength of the L1 sparsity loss returned by forward. Default 5e-4.
        active_flag (bool): interpolate on the forward pass (active shift). Default False.
        emulate_dw (dict): parameters of the depthwise conv this layer replaces (kernel_size,
            stride, padding, padding_mode); output cropping / pooling are derived from them.
        init_thumb_rule (int): 1: uniform(-init_shift, init_shift); 2: uniform(0, init_shift) * sign.
    """
    dim = None

    @staticmethod
    def _identity(x):
        return x

    @staticmethod
    def _pooling(ks, dim):
        if isinstance(ks, torch.Tensor):
            ks = ks.squeeze().cpu().numpy().tolist()
        return partial(_AVG_POOLS[min(dim, 3)], kernel_size=ks, stride=ks, ceil_mode=True)

    @staticmethod
    def _init_thumb_rule_1(size, shape):
        return 2 * size * torch.rand(shape) - size

    @staticmethod
    def _init_thumb_rule_2(size, shape):
        return size * torch.rand(shape) * (1 if random.random() < 0.5 else -1)

    def __init__(self, in_channels, padding='zeros', init_shift=1, sparsity_term=5e-4, active_flag=False,
                 emulate_dw=None, init_thumb_rule=1):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        self.padding = paddings_dict[padding]
        self.sparsity_term = sparsity_term
        self.in_channels = in_channels
        self._active_flag = active_flag
        self._shift_func = self._init_shift_fn()
        self.cut_borders = None
        self._reduction_fn = self._identity
        self._pool_size = None  # window (= stride) of the average pool that follows the shift, when there is one
        # QUIRK (reference modules/shifts.py:117-118): rule 2 is selected with `==` instead of `=`,
        # so both rule numbers initialise with rule 1.  Kept: initial weights match the reference.
        self._w_init_func = self._init_thumb_rule_1
        self.init_shift = torch.tensor(_wrap_dim(init_shift, self.dim, 'init_shift'), requires_grad=False)
        self._w_post_init_scale = torch.ones(1, self.dim, requires_grad=False)

        if emulate_dw is not None:
            emulate_dw['init_thumb_rule_type'] = init_thumb_rule  # QUIRK: the caller's dict is modified (:125)
            self.init_shift, self._w_post_init_scale, self.cut_borders, _conv_padding = \
                _create_dw_emulation(emulate_dw, self.dim)
            # QUIRK (:128-129): the conv's padding_mode is compared, not assigned -> self.padding is unchanged.
            if not (self._w_post_init_scale == 1).all():
                self._reduction_fn = self._pooling(self._w_post_init_scale, self.dim)
                self._pool_size = [int(k) for k in self._w_post_init_scale.reshape(-1).tolist()]
        self._init_weights()

    def _init_shift_fn(self):
        if self.dim not in _SHIFT_FUNCS:
            raise NotImplementedError
        return _SHIFT_FUNCS[self.dim]

    def _init_weights(self):
        self.weight = nn.Parameter(torch.Tensor(self.in_channels, self.dim))
        self.reset_parameters()

    def reset_parameters(self):
        for i in range(self.dim):
            self.weight.data[:, i] = self._w_init_func(self.init_shift[i], self.in_channels)
        self.weight.data *= self._w_post_init_scale

    def _compute_weight_loss(self):
        return self.sparsity_term * torch.sum(torch.abs(self.weight))

    def forward(self, input):
        """Returns (output, loss); loss is None when sparsity_term == 0."""
        loss = self._compute_weight_loss() if bool(self.sparsity_term) else None
        if self._pool_size is not None and self.dim in _SHIFT_POOL_FUNCS:
            # reference: self._reduction_fn(shift(x)) (modules/shifts.py:150-153).  Same values from one op: on HIP
            # tensors the shift output is pooled on the fly instead of being written and re-read
            return _SHIFT_POOL_FUNCS[self.dim](input, self.weight, self.padding, self._active_flag, self.cut_borders,
                                               self._pool_size), loss
        out = self._shift_func(input, self.weight, self.padding, self._active_flag, self.cut_borders)
        return self._reduction_fn(out), loss

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        active = f'Active shift on forward pass: {"Yes" if self._active_flag else "No"}'
        sparse = ('Sparse shift: Yes - sparsity strength: {}'.format(self.sparsity_term)
                  if bool(self.sparsity_term) else 'Sparse shift: No')
        return f'in_channels={self.in_channels}, padding_method={pad}, {active}, {sparse}'


class Shift1d(_Shiftnd):
    """Learnable per-channel shift of a [N, C, H] tensor (zero-FLOP stand-in for a depthwise conv).
    forward(x) -> (out, loss).  Arguments: see _Shiftnd."""
    dim = 1


class Shift2d(_Shiftnd):
    """Learnable per-channel (H, W) shift of a [N, C, H, W] tensor.  forward(x) -> (out, loss)."""
    dim = 2


class Shift3d(_Shiftnd):
    """Learnable per-channel (H, W, D) shift of a [N, C, H, W, D] tensor.  forward(x) -> (out, loss)."""
    dim = 3


class _GroupedShiftnd(nn.Module):
    """Fixed integer shifts, nothing to learn (GroupedShift, arXiv 1711.08141 section 3.1; or a trained sparse-shift layer frozen
    by `from_shift`).  The table is the persistent buffer `shifts` (int64 [in_channels, dim]): it travels in state_dict and with
    .to(device), and the module has no parameters.  The backward returns the input gradient alone: the autograd node keeps the
    table, never the input, and no weight gradient is computed.

    Arguments:
        in_channels (int): channels of the input.
        kernel_size (int): the default table splits the channels, in order, into kernel_size**dim equal groups; group g is
            shifted by unravel(g, (kernel_size,) * dim) - kernel_size // 2, the in_channels % kernel_size**dim channels left
            over are not shifted.  Default 3.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        shifts (tensor / nested list): a [in_channels, dim] table of integers that replaces the default one.
        emulate_dw (dict): parameters of the depthwise conv this layer replaces (kernel_size, stride, padding): the output is
            cut as Shift{N}d cuts it, and with a stride > 1 followed by the same avg_pool{N}d(ceil_mode=True), shift and pool as
            one op (shift{N}d_fixed_pool: on HIP tensors fused in both directions); its kernel_size also sizes the default table.
    forward(x) -> (output, None): the pair convention of Shift{N}d with sparsity_term == 0.
    """
    dim = None

    def __init__(self, in_channels, kernel_size=3, padding='zeros', shifts=None, emulate_dw=None):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        self.padding = paddings_dict[padding.lower()]
        self.in_channels = in_channels
        self.cut_borders = None
        self._pool_size = None
        if emulate_dw is not None:
            args = dict(emulate_dw)   # (the caller's dict stays as it is)
            args.setdefault('init_thumb_rule_type', 1)
            _, scales, self.cut_borders, _ = _create_dw_emulation(args, self.dim)
            if not (scales == 1).all():
                self._pool_size = [int(k) for k in scales.reshape(-1).tolist()]
            kernel_size = _wrap_dim(args['kernel_size'], self.dim, 'kernel_size')[0]
        self.kernel_size = int(kernel_size)
        if shifts is None:
            table = self.default_table(in_channels, self.kernel_size, self.dim)
        else:
            table = torch.as_tensor(shifts)
            assert tuple(table.shape) == (in_channels, self.dim), f'shifts must have shape [{in_channels}, {self.dim}]'
            if table.is_floating_point():
                table = torch.round(table)
            table = table.detach().to(torch.int64).clone()
        self.register_buffer('shifts', table, persistent=True)

    @staticmethod
    def default_table(in_channels, kernel_size, dim):
        groups = kernel_size ** dim
        per = in_channels // groups
        table = torch.zeros(in_channels, dim, dtype=torch.int64)
        if per > 0:
            g = torch.arange(groups * per) // per
            for d in range(dim):
                table[:groups * per, d] = (g // kernel_size ** (dim - 1 - d)) % kernel_size - kernel_size // 2
        return table

    @classmethod
    def from_shift(cls, module):
        """Freeze a trained, non-active Shift{N}d: round(weight) (half to even, the kernels' rounding), its padding, cut borders
        and pool tail."""
        assert isinstance(module, _Shiftnd) and module.dim == cls.dim, f'expected a Shift{cls.dim}d module'
        if module._active_flag:
            raise ValueError('an active shift interpolates: it cannot be frozen into integer shifts')
        pad = {v: k for k, v in paddings_dict.items()}[module.padding]
        table = torch.round(module.weight.detach()).to(torch.int64)
        frozen = cls(module.in_channels, padding=pad, shifts=table.cpu())
        frozen.cut_borders = None if module.cut_borders is None else module.cut_borders.clone()
        frozen._pool_size = None if module._pool_size is None else list(module._pool_size)
        return frozen.to(module.weight.device)

    def forward(self, input):
        """Returns (output, None)."""
        if self._pool_size is not None:
            return _SHIFT_FIXED_POOL_FUNCS[self.dim](input, self.shifts, self.padding, self._pool_size, self.cut_borders), None
        return _SHIFT_FIXED_FUNCS[self.dim](input, self.shifts, self.padding, self.cut_borders), None

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        return f'in_channels={self.in_channels}, kernel_size={self.kernel_size}, padding_method={pad}, fixed integer shifts'


class GroupedShift1d(_GroupedShiftnd):
    """Fixed per-channel shift of a [N, C, H] tensor.  forward(x) -> (out, None).  Arguments: see _GroupedShiftnd."""
    dim = 1


class GroupedShift2d(_GroupedShiftnd):
    """Fixed per-channel (H, W) shift of a [N, C, H, W] tensor.  forward(x) -> (out, None)."""
    dim = 2


class GroupedShift3d(_GroupedShiftnd):
    """Fixed per-channel (H, W, D) shift of a [N, C, H, W, D] tensor.  forward(x) -> (out, None)."""
    dim = 3


class TemporalShift(nn.Module):
    """Temporal Shift Module (arXiv 1811.08383): fixed shifts across the frames of a [N * n_segment, C, ...] tensor, nothing to
    learn.  The table is the persistent buffer `shifts` (int64 [in_channels]): channel c of frame t becomes channel c of frame
    t - shifts[c] of the same clip.  It travels in state_dict and with .to(device); the module has no parameters, and the autograd
    node keeps the table alone.

    Arguments:
        n_segment (int): frames per clip, T.
        in_channels (int): channels of the input.
        fold_div (int): the default table moves the first in_channels // fold_div channels one frame back (shift -1: frame t
            shows frame t + 1), the next in_channels // fold_div one frame forward (+1) and leaves the rest. Default 8.
        shifts (tensor / list): [in_channels] integers that replace the default table (fold_div is then unused); floats are
            rounded half to even, not validated.  On HIP tensors |shift| <= 256 is exact in bfloat16, <= 2048 in float16.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros' (the published module).
        memory_format: torch.contiguous_format (default: a contiguous output) or torch.preserve_format (a dense channels-last
            input comes back channels-last, shifted as it lies on HIP tensors: for channels-last models).  A plain attribute,
            not part of state_dict.
        inplace (bool): shift the input itself and return it (the published InplaceShift): on HIP tensors a dense input of at
            most 16 frames per clip is one pass over the shifted channels alone, without an output allocation.  memory_format is
            then moot, the layout being the input's own.  A plain attribute, not part of state_dict. Default False.
    forward(x) -> output, the tensor alone: the module sits inside nn.Sequential in front of a convolution.
    """

    def __init__(self, n_segment, in_channels, fold_div=8, shifts=None, padding='zeros', memory_format=torch.contiguous_format,
                 inplace=False):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        assert memory_format in (torch.contiguous_format, torch.preserve_format), \
            f'memory_format must be torch.contiguous_format or torch.preserve_format, not {memory_format}'
        self.memory_format = memory_format
        self.inplace = bool(inplace)
        self.padding = paddings_dict[padding.lower()]
        self.n_segment = int(n_segment)
        self.in_channels = in_channels
        self.fold_div = int(fold_div)
        if shifts is None:
            table = self.default_table(in_channels, self.fold_div)
        else:
            table = torch.as_tensor(shifts)
            assert tuple(table.shape) == (in_channels,), f'shifts must have shape [{in_channels}]'
            if table.is_floating_point():
                table = torch.round(table)
            table = table.detach().to(torch.int64).clone()
        self.register_buffer('shifts', table, persistent=True)

    @staticmethod
    def default_table(in_channels, fold_div):
        fold = in_channels // fold_div
        table = torch.zeros(in_channels, dtype=torch.int64)
        table[:fold] = -1
        table[fold:2 * fold] = 1
        return table

    @classmethod
    def from_shift(cls, module):
        """Freeze a trained, non-active LearnableTemporalShift: round(weight) (half to even, the kernels' rounding), its n_segment
        and padding.  Output and input gradient are the learnable module's, bit for bit."""
        assert isinstance(module, LearnableTemporalShift), 'expected a LearnableTemporalShift module'
        if module._active_flag:
            raise ValueError('an active shift interpolates: it cannot be frozen into integer shifts')
        pad = {v: k for k, v in paddings_dict.items()}[module.padding]
        table = torch.round(module.weight.detach().reshape(-1)).to(torch.int64)
        return cls(module.n_segment, module.in_channels, shifts=table.cpu(), padding=pad).to(module.weight.device)

    def forward(self, input):
        if self.inplace:
            return temporal_shift_func_(input, self.shifts, self.n_segment, self.padding)
        return temporal_shift_func(input, self.shifts, self.n_segment, self.padding, self.memory_format)

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        return (f'n_segment={self.n_segment}, in_channels={self.in_channels}, fold_div={self.fold_div}, padding_method={pad}, '
                f'memory_format={self.memory_format}, fixed integer shifts' + (', inplace=True' if self.inplace else ''))


class OnlineTemporalShift(nn.Module):
    """Online Temporal Shift Module (the uni-directional TSM of arXiv 1811.08383, section 4.2): frames of B independent streams
    arrive one at a time as [B, C, ...], and the channels that shift are taken from a cache of the previous frames.  The table is the
    persistent buffer `shifts` (int64 [in_channels], every entry >= 0): channel c of the frame at time t shows channel c of the frame
    at time t - shifts[c].  Fed the frames of a clip one by one, the module returns, stacked, what TemporalShift returns for the clip
    under the same table and padding.  Inference only: a frame that requires grad raises.

    Arguments:
        in_channels (int): channels of the frames.
        fold_div (int): the default table shows the first in_channels // fold_div channels one frame late (shift 1) and leaves the
            rest. Default 8.
        shifts (tensor / list): [in_channels] integers >= 0 that replace the default table (fold_div is then unused).
        padding (str): 'zeros' | 'border': what the first frames see in place of the frames before the stream began -- zeros (the
            zero point of a quantized frame), or the first frame.  The other paddings look into the future and are refused.
        inplace (bool): shift the frame itself and return it; otherwise a clone is shifted.  A plain attribute, not part of
            state_dict. Default False.
    forward(frame) -> the shifted frame alone.  The state ([max(shifts), B, C, ...] in the frame's layout) is the plain attribute
    `state`, not part of state_dict: it is made on the first call (torchshifts.functional.temporal_shift_online_state: the one host
    synchronisation) and dropped by reset(), which starts a new stream.  A later frame of another shape, dtype, device or layout
    raises.  On HIP tensors a step on a dense frame with max(shifts) <= 15 is one kernel over the shifted channels alone, with no
    allocation (inplace=True) and no host synchronisation: it can be captured in a torch.cuda.graph once the state exists.
    """
    def __init__(self, in_channels, fold_div=8, shifts=None, padding='zeros', inplace=False):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        if paddings_dict[padding.lower()] > 1:
            raise ValueError(f'{padding} padding looks into the future: an online shift pads with zeros or border')
        self.padding = paddings_dict[padding.lower()]
        self.inplace = bool(inplace)
        self.in_channels = in_channels
        self.fold_div = int(fold_div)
        if shifts is None:
            table = self.default_table(in_channels, self.fold_div)
        else:
            table = torch.as_tensor(shifts)
            assert tuple(table.shape) == (in_channels,), f'shifts must have shape [{in_channels}]'
            if table.is_floating_point():
                table = torch.round(table)
            table = table.detach().to(torch.int64).clone()
            if table.numel() and int(table.min()) < 0:
                raise ValueError('a negative shift reads the future: an online table is causal (every entry >= 0)')
        self.register_buffer('shifts', table, persistent=True)
        self.state = None
        self._table = None   # `shifts` in the kind the kernel reads: made with the state
        self._frame = None   # shape, strides, dtype and device of the frames the state was made for

    @staticmethod
    def default_table(in_channels, fold_div):
        table = torch.zeros(in_channels, dtype=torch.int64)
        table[:in_channels // fold_div] = 1
        return table

    @classmethod
    def from_shift(cls, module, inplace=False):
        """The online form of a TemporalShift whose table is causal (every entry >= 0), with its padding; ValueError otherwise --
        the published bidirectional table reads one frame ahead."""
        assert isinstance(module, TemporalShift), 'expected a TemporalShift module'
        table = module.shifts.detach().cpu()
        if table.numel() and int(table.min()) < 0:
            raise ValueError('the table reads the future (a negative shift): no online form')
        pad = {v: k for k, v in paddings_dict.items()}[module.padding]
        return cls(module.in_channels, fold_div=module.fold_div, shifts=table, padding=pad, inplace=inplace).to(module.shifts.device)

    def reset(self):
        """Drop the state: the next frame begins a new stream."""
        self.state = None
        self._table = None
        self._frame = None

    def _step(self, frame, state, table):
        return (temporal_shift_online_func_ if self.inplace else temporal_shift_online_func)(frame, state, table)

    def forward(self, input):
        if self.state is None:
            self.state = temporal_shift_online_state(input, self.shifts, self.padding)
            self._table = temporal_shift_online_table(input, self.shifts)
            self._frame = (tuple(input.shape), tuple(input.stride()), input.dtype, input.device)
        else:
            frame = (tuple(input.shape), tuple(input.stride()), input.dtype, input.device)
            if frame != self._frame:
                raise RuntimeError('OnlineTemporalShift: the state was made for frames of shape %s, strides %s, %s on %s, but this frame '
                                   'has shape %s, strides %s, %s on %s; reset() starts a new stream' % (self._frame + frame))
        return self._step(input, self.state, self._table)

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        return (f'in_channels={self.in_channels}, fold_div={self.fold_div}, padding_method={pad}, fixed integer shifts, online'
                + (', inplace=True' if self.inplace else ''))


class LearnableTemporalShift(nn.Module):
    """Learnable per-channel shift across the frames of a [N * n_segment, C, ...] tensor: Shift1d along the frames of each clip
    (the temporal half of learnable-shift video models), without a layout change.  `weight` is a [in_channels, 1] parameter,
    initialised like Shift1d's; with active_flag the forward interpolates between two frames, without it the shift is
    round(weight) and TemporalShift.from_shift freezes the trained layer into the fixed module.

    Arguments:
        n_segment (int): frames per clip, T.
        in_channels (int): channels of the input.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        init_shift (float): bound of the uniform weight initialisation. Default 1.
        sparsity_term (float): strength of the L1 sparsity loss returned by forward. Default 5e-4.
        active_flag (bool): interpolate on the forward pass (active shift). Default False.
        init_thumb_rule (int): as Shift1d's (both values initialise with uniform(-init_shift, init_shift)).
        memory_format: torch.contiguous_format (default: a contiguous output) or torch.preserve_format (a dense channels-last
            input comes back channels-last, served as it lies on HIP tensors, forward and backward).  A plain attribute, not
            part of the state_dict.
    forward(x) -> (output, loss): the pair convention of Shift{N}d; loss is None when sparsity_term == 0.
    """

    def __init__(self, n_segment, in_channels, padding='zeros', init_shift=1, sparsity_term=5e-4, active_flag=False,
                 init_thumb_rule=1, memory_format=torch.contiguous_format):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        assert memory_format in (torch.contiguous_format, torch.preserve_format), \
            f'memory_format must be torch.contiguous_format or torch.preserve_format, not {memory_format}'
        self.memory_format = memory_format
        self.padding = paddings_dict[padding.lower()]
        self.n_segment = int(n_segment)
        self.in_channels = in_channels
        self.sparsity_term = sparsity_term
        self._active_flag = active_flag
        self.init_shift = torch.tensor(_wrap_dim(init_shift, 1, 'init_shift'), requires_grad=False)
        self.weight = nn.Parameter(torch.Tensor(in_channels, 1))
        self.reset_parameters()

    def reset_parameters(self):
        self.weight.data[:, 0] = _Shiftnd._init_thumb_rule_1(self.init_shift[0], self.in_channels)

    def _compute_weight_loss(self):
        return self.sparsity_term * torch.sum(torch.abs(self.weight))

    def forward(self, input):
        """Returns (output, loss); loss is None when sparsity_term == 0."""
        loss = self._compute_weight_loss() if bool(self.sparsity_term) else None
        return temporal_shift_learnable_func(input, self.weight, self.n_segment, self.padding, self._active_flag,
                                             self.memory_format), loss

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        active = f'Active shift on forward pass: {"Yes" if self._active_flag else "No"}'
        sparse = ('Sparse shift: Yes - sparsity strength: {}'.format(self.sparsity_term)
                  if bool(self.sparsity_term) else 'Sparse shift: No')
        return (f'n_segment={self.n_segment}, in_channels={self.in_channels}, padding_method={pad}, {active}, {sparse}, '
                f'memory_format={self.memory_format}')


class PerClipTemporalShift(nn.Module):
    """Fixed shifts across the frames of a [N * n_segment, C, ...] tensor under a table that differs from clip to clip: channel c
    of frame t of clip n becomes channel c of frame t - table[n, c] of the same clip (per-clip temporal jitter; the integer
    offsets of a net that looks at the clip).  The module has no parameter and no buffer: the table comes from the caller, and
    the autograd node keeps it alone.

    Arguments:
        n_segment (int): frames per clip, T.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        memory_format: torch.contiguous_format (default: a contiguous output) or torch.preserve_format (a dense channels-last
            input comes back channels-last; on the GPU it is shifted as it lies, without a layout change).  Choose it with a group
            table [N, G] whose groups span whole 16-byte pieces of a pixel's channel row (8 fp16 / 4 fp32 channels or more); under
            an ungrouped [N, C] table keep the default, whose backward is faster although it changes the layout twice.
    forward(x, table) -> output, the tensor alone.  table: [N, C] integers (floats are rounded half to even), or [N, G] with
    C % G == 0, entry g serving the C // G consecutive channels of group g.
    """

    def __init__(self, n_segment, padding='zeros', memory_format=torch.contiguous_format):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        assert memory_format in (torch.contiguous_format, torch.preserve_format), \
            f'memory_format must be torch.contiguous_format or torch.preserve_format, not {memory_format}'
        self.padding = paddings_dict[padding.lower()]
        self.n_segment = int(n_segment)
        self.memory_format = memory_format

    def forward(self, input, table):
        return temporal_shift_per_clip_func(input, table, self.n_segment, self.padding, self.memory_format)

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        fmt = '' if self.memory_format == torch.contiguous_format else f', memory_format={self.memory_format}'
        return f'n_segment={self.n_segment}, padding_method={pad}, per-clip integer shifts' + fmt


class LearnablePerClipTemporalShift(nn.Module):
    """Differentiable shifts across the frames of a [N * n_segment, C, ...] tensor under a table that a net predicts from the clip
    itself (the Temporal Interlacing Network's OffsetNet, arXiv 2001.06499): clip n is shifted by table[n], sparse (rounded) or,
    with active_flag, interpolated between two frames; the gradient flows into the input and into the table, hence into the
    net that produced it.  The module has no parameter and no buffer.

    Arguments:
        n_segment (int): frames per clip, T.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        active_flag (bool): interpolate on the forward pass (active shift). Default False.
        memory_format: torch.contiguous_format (default: a contiguous output) or torch.preserve_format (a dense channels-last
            input comes back channels-last, x.grad in the layout of the incoming gradient; on the GPU both passes run on the
            tensors as they lie).
    forward(x, table) -> output, the tensor alone.  table: [N, C] floats of the input's dtype (float32 with a float16 / bfloat16
    input works too), or [N, G] with C % G == 0 (TIN's groups): a group's gradient is the sum over its channels.
    """

    def __init__(self, n_segment, padding='zeros', active_flag=False, memory_format=torch.contiguous_format):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        assert memory_format in (torch.contiguous_format, torch.preserve_format), \
            f'memory_format must be torch.contiguous_format or torch.preserve_format, not {memory_format}'
        self.padding = paddings_dict[padding.lower()]
        self.n_segment = int(n_segment)
        self._active_flag = active_flag
        self.memory_format = memory_format

    def forward(self, input, table):
        return temporal_shift_learnable_per_clip_func(input, table, self.n_segment, self.padding, self._active_flag,
                                                      self.memory_format)

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        active = f'Active shift on forward pass: {"Yes" if self._active_flag else "No"}'
        fmt = '' if self.memory_format == torch.contiguous_format else f', memory_format={self.memory_format}'
        return f'n_segment={self.n_segment}, padding_method={pad}, {active}, per-clip weights' + fmt


class OffsetNet(nn.Module):
    """TIN's offset predictor (arXiv 2001.06499): a clip's descriptor [N, fold, T] -> two offsets per clip in (-2, 2), [N, 2].
    Conv1d(fold, 1, 3, padding=1) -> [N, T] -> Linear(T, T) -> ReLU -> Linear(T, 2) -> 4 * (sigmoid - 0.5); the last Linear's bias
    starts at 0.5108."""

    def __init__(self, in_channels, n_segment):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, 1, 3, padding=1)
        self.fc1 = nn.Linear(n_segment, n_segment)
        self.fc2 = nn.Linear(n_segment, 2)
        nn.init.constant_(self.fc2.bias, 0.5108)

    def forward(self, desc):
        h = self.conv(desc).view(desc.shape[0], desc.shape[2])
        return 4 * (torch.sigmoid(self.fc2(torch.relu(self.fc1(h)))) - 0.5)


class WeightNet(nn.Module):
    """TIN's weight predictor: a clip's descriptor [N, fold, T] -> two weights per clip and frame in (0, 2), [N, T, 2].
    Conv1d(fold, 2, 3, padding=1) -> permute -> 2 * sigmoid; the Conv1d's bias starts at 0."""

    def __init__(self, in_channels):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, 2, 3, padding=1)
        nn.init.constant_(self.conv.bias, 0.0)

    def forward(self, desc):
        return 2 * torch.sigmoid(self.conv(desc).permute(0, 2, 1))


class TemporalInterlace(nn.Module):
    """The Temporal Interlacing layer (TIN, arXiv 2001.06499) on a [N * n_segment, C, ...] tensor: an OffsetNet and a WeightNet look
    at the spatial mean of the first fold = in_channels // shift_div channels of each clip and predict two offsets o [N, 2] and two
    per-frame weights w [N, T, 2]; the four channel groups of the fold are shifted by (o, -o) -- the published sampler reads
    x[t + offset] -- interpolating between two frames, and weighted by (w, w); channels from fold up pass through (offset 0,
    weight 1).  The whole layer is ONE temporal_interlace_func call on the whole tensor: no slice and no cat of the activation.

    Arguments:
        n_segment (int): frames per clip, T.
        in_channels (int): C.
        shift_div (int): the first C // shift_div channels are interlaced. Default 1 (all of them).
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        memory_format: torch.contiguous_format (default: a contiguous output) or torch.preserve_format (a dense channels-last
            input comes back channels-last; on the GPU one kernel per pass on the tensor as it lies -- the layer's own tables
            are the frame kernels' fast path).  A plain attribute, not part of state_dict.
    forward(x) -> output, the tensor alone.
    """

    def __init__(self, n_segment, in_channels, shift_div=1, padding='zeros', memory_format=torch.contiguous_format):
        super().__init__()
        assert padding.lower() in paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        assert memory_format in (torch.contiguous_format, torch.preserve_format), \
            f'memory_format must be torch.contiguous_format or torch.preserve_format, not {memory_format}'
        self.memory_format = memory_format
        self.n_segment = int(n_segment)
        self.in_channels = int(in_channels)
        self.shift_div = int(shift_div)
        self.fold = self.in_channels // self.shift_div
        assert self.fold >= 4 and self.fold % 4 == 0, \
            f'in_channels // shift_div ({self.fold}) must be a positive multiple of 4: the fold holds four channel groups'
        self.padding = paddings_dict[padding.lower()]
        self.offset_net = OffsetNet(self.fold, self.n_segment)
        self.weight_net = WeightNet(self.fold)

    def tables(self, input):
        """offsets [N, C] and scales [N, T, C] of the one call, from the nets' [N, 2] and [N, T, 2]"""
        T, C, fold = self.n_segment, self.in_channels, self.fold
        N = input.shape[0] // T
        desc = input[:, :fold].reshape(N, T, fold, -1).mean(3).permute(0, 2, 1).to(self.offset_net.conv.weight.dtype)
        o, w = self.offset_net(desc), self.weight_net(desc)
        table, weight = torch.cat((o, -o), 1), torch.cat((w, w), 2)          # [N, 4], [N, T, 4]
        offsets = (-table).repeat_interleave(fold // 4, dim=1)               # (the op's sign: out[t] = x[t - w])
        scales = weight.repeat_interleave(fold // 4, dim=2)
        if fold < C:
            offsets = torch.cat((offsets, offsets.new_zeros(N, C - fold)), 1)
            scales = torch.cat((scales, scales.new_ones(N, T, C - fold)), 2)
        kind = torch.float32 if input.dtype in (torch.float16, torch.bfloat16) else input.dtype
        return offsets.to(kind), scales.to(kind)

    def forward(self, input):
        assert input.shape[1] == self.in_channels and input.shape[0] % self.n_segment == 0, \
            f'expected a [N * {self.n_segment}, {self.in_channels}, ...] tensor, but it is shape is {tuple(input.shape)}'
        offsets, scales = self.tables(input)
        return temporal_interlace_func(input, offsets, scales, self.n_segment, self.padding, True, self.memory_format)

    def extra_repr(self):
        pad = {v: k for k, v in paddings_dict.items()}[self.padding]
        fmt = '' if self.memory_format == torch.contiguous_format else f', memory_format={self.memory_format}'
        return f'n_segment={self.n_segment}, in_channels={self.in_channels}, shift_div={self.shift_div}, padding_method={pad}' + fmt
