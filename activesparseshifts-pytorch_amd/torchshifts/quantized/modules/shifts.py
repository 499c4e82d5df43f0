"""Quantized shift modules (reference torchshifts/quantized/modules/shifts.py).

`forward` returns the tensor only (no loss).  `from_float` converts a float Shift{N}d; the integer
shifts are `int_repr(qweight) - zero_point`, the scale is not used by the kernel
(kernels/shifts_kernels.h:553-555).

Differences from the reference:
  * the quantized weights checkpoint and move with the module: their integer representation is a buffer
    (`qweight_repr`), scale / zero point / dtype travel as the module's extra state; `qweight` is a property that
    rebuilds the quantized tensor on the buffer's device (the reference keeps a plain attribute, :17, that
    `state_dict()` drops and `.to(device)` leaves behind);
  * `quantize_shift_weights` never changes a shift: the reference's `scale = ceil(range / 255)` (:10-12) is 0 when all
    weights are equal (torch raises) and > 1 when the range exceeds 255, which silently HALVES every shift because
    the kernel ignores the scale.  Here the scale is always 1; weights that do not fit quint8 around zero point 128
    (|round(w)| > 127) become qint32 with zero point 0, which both backends accept.
"""
import copy
import warnings

import torch

import torchshifts.modules.shifts as shifts
from torchshifts.functional import shift1d_pool_func, shift2d_pool_func, shift3d_pool_func
from torchshifts.quantized.functional import shift1d_quantized, shift2d_quantized, shift3d_quantized, temporal_shift_quantized, temporal_shift_quantized_, temporal_shift_online_quantized, temporal_shift_online_quantized_, temporal_shift_learnable_quantized, temporal_interlace_quantized, temporal_shift_learnable_per_clip_quantized

_POOL_FUNCS = {1: shift1d_pool_func, 2: shift2d_pool_func, 3: shift3d_pool_func}

rp_dict = {v: k for k, v in shifts.paddings_dict.items()}


def quantize_shift_weights(weight):
    """Float shift weights -> quantized tensor whose `int_repr - zero_point` is round-half-even(weight).

    quint8, scale 1, zero point 128 (the reference's layout whenever the reference is right); qint32, scale 1, zero
    point 0 when a rounded shift leaves [-128, 127]."""
    w = weight.detach().float()
    if w.numel() and not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_shift_weights: weights must be finite")
    amax = float(w.abs().max()) if w.numel() else 0.0
    if amax <= 127.0:
        return torch.quantize_per_tensor(w, 1.0, 128, torch.quint8)
    warnings.warn("shift weights beyond +-127 do not fit quint8 around zero point 128: using qint32 weights "
                  "(the reference would have coarsened every shift by ceil(range / 255))", stacklevel=2)
    return torch.quantize_per_tensor(w, 1.0, 0, torch.qint32)


class _QuantizedShiftMixin:
    _qfunc = None
    _qname = None

    def _init_quantized(self):
        self.register_buffer("qweight_repr", torch.zeros(self.in_channels, self.dim, dtype=torch.uint8))
        self._q_scale, self._q_zero_point, self._q_dtype = 1.0, 128, "quint8"
        self.qweight = quantize_shift_weights(self.weight.float())

    # ---- the quantized weights: buffer + extra state ---------------------------------------------------------
    @property
    def qweight(self):
        return torch._make_per_tensor_quantized_tensor(self.qweight_repr, self._q_scale, self._q_zero_point)

    @qweight.setter
    def qweight(self, q):
        if not q.is_quantized:
            raise ValueError("qweight must be a per-tensor quantized tensor")
        self._q_scale, self._q_zero_point = float(q.q_scale()), int(q.q_zero_point())
        self._q_dtype = str(q.dtype).replace("torch.", "")
        self.qweight_repr = q.int_repr()  # (an existing buffer name: nn.Module keeps it registered)

    def get_extra_state(self):
        return {"qweight_scale": self._q_scale, "qweight_zero_point": self._q_zero_point, "qweight_dtype": self._q_dtype}

    def set_extra_state(self, state):
        self._q_scale = float(state["qweight_scale"])
        self._q_zero_point = int(state["qweight_zero_point"])
        self._q_dtype = state["qweight_dtype"]
        want = {"quint8": torch.uint8, "qint8": torch.int8, "qint32": torch.int32}[self._q_dtype]
        if self.qweight_repr.dtype != want:  # load_state_dict copies INTO the existing buffer: give it the saved type
            self.qweight_repr = self.qweight_repr.to(want)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key, extra = prefix + "qweight_repr", prefix + "_extra_state"
        legacy = key not in state_dict and (prefix + "weight") in state_dict
        if key in state_dict and state_dict[key].dtype != self.qweight_repr.dtype:
            self.qweight_repr = torch.zeros_like(self.qweight_repr, dtype=state_dict[key].dtype)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if legacy:
            # a checkpoint in the reference's layout (only the float `weight`: its `qweight` is a plain attribute that
            # state_dict() drops, quantized/modules/shifts.py:17): the quantized weights are what from_float would make
            # of the loaded float weights -- never the fresh module's initial shifts
            self.qweight = quantize_shift_weights(self.weight.detach().float())
            for k in (key, extra):
                while k in missing_keys:
                    missing_keys.remove(k)

    def forward(self, input):
        if self._pool_size is not None and input.is_cuda:
            # ATen has no QuantizedCUDA average pool: torchshifts::shift{N}d_pool on the QuantizedCUDA key runs the shift and
            # the pool as one pass (int8 / uint8) with the QuantizedCPU pool's arithmetic -- the values _reduction_fn gives
            # on CPU tensors, ragged last windows included
            if not input.is_quantized:
                raise ValueError(f"Input to '{self._qname}' must be quantized!")
            return _POOL_FUNCS[self.dim](input, self.qweight, self.padding, False, self.cut_borders, self._pool_size)
        out = type(self)._qfunc(input, self.qweight, self.padding, self.cut_borders)
        return self._reduction_fn(out)

    def _get_name(self):
        return self._qname

    @classmethod
    def from_float(cls, mod):
        qshift = cls(mod.in_channels, rp_dict[mod.padding])
        qshift.cut_borders = mod.cut_borders
        qshift._reduction_fn = mod._reduction_fn
        qshift._pool_size = getattr(mod, "_pool_size", None)
        qshift.weight = mod.weight
        qshift.qweight = quantize_shift_weights(mod.weight.float())
        return qshift


class Shift1d(_QuantizedShiftMixin, shifts.Shift1d):
    _qfunc = staticmethod(shift1d_quantized)
    _qname = 'QuantizedShift1D'

    def __init__(self, in_channels, padding='zeros'):
        super().__init__(in_channels, padding, 1, 0, False)
        self._init_quantized()


class Shift2d(_QuantizedShiftMixin, shifts.Shift2d):
    _qfunc = staticmethod(shift2d_quantized)
    _qname = 'QuantizedShift2D'

    def __init__(self, in_channels, padding='zeros'):
        super().__init__(in_channels, padding, 1, 0, False)
        self._init_quantized()


class Shift3d(_QuantizedShiftMixin, shifts.Shift3d):
    _qfunc = staticmethod(shift3d_quantized)
    _qname = 'QuantizedShift3D'

    def __init__(self, in_channels, padding='zeros'):
        super().__init__(in_channels, padding, 1, 0, False)
        self._init_quantized()


class TemporalShift(shifts.TemporalShift):
    """Quantized Temporal Shift Module: the float TemporalShift on per-tensor quantized tensors (quint8, qint8, qint32).  The table
    is the same persistent int64 buffer `shifts`, so a float TemporalShift checkpoint loads as it is; there are no quantized
    weights, because the table holds integers already.  The output keeps the input's scale and zero point, and zeros padding
    fills with the zero point.  On HIP tensors the table is passed as int32: every shift is exact.

    forward(x) -> output, the tensor alone.  from_float converts a TemporalShift, or a non-active LearnableTemporalShift
    (frozen through TemporalShift.from_shift: round(weight), half to even); an active one interpolates and raises ValueError.
    memory_format is the float module's option (torch.preserve_format: a channels-last input comes back channels-last);
    from_float carries the float module's value over, and that of `inplace` (the input itself is shifted and returned).
    """

    def forward(self, input):
        if self.inplace:
            return temporal_shift_quantized_(input, self.shifts, self.n_segment, self.padding)
        return temporal_shift_quantized(input, self.shifts, self.n_segment, self.padding, self.memory_format)

    def _get_name(self):
        return 'QuantizedTemporalShift'

    @classmethod
    def from_float(cls, mod):
        if isinstance(mod, shifts.LearnableTemporalShift):
            mod = shifts.TemporalShift.from_shift(mod)
        assert isinstance(mod, shifts.TemporalShift), 'expected a TemporalShift or LearnableTemporalShift module'
        qshift = cls(mod.n_segment, mod.in_channels, fold_div=mod.fold_div, shifts=mod.shifts.detach().cpu(), padding=rp_dict[mod.padding],
                     memory_format=mod.memory_format, inplace=mod.inplace)
        return qshift.to(mod.shifts.device)


class LearnableTemporalShift(torch.nn.Module):
    """Quantized learnable Temporal Shift Module: the float LearnableTemporalShift on per-tensor quantized tensors (quint8, qint8,
    qint32), interpolating in the integer domain (torchshifts.quantized.functional.temporal_shift_learnable_quantized).  `weight`
    is a persistent fp32 buffer [in_channels, 1] -- the trained shifts as they are, never rounded under active_flag -- so a float
    LearnableTemporalShift checkpoint's `weight` loads.  The output keeps the input's scale and zero point and is contiguous.

    Arguments:
        n_segment (int): frames per clip, T.
        in_channels (int): channels of the input.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        active_flag (bool): interpolate between two frames. Default True; without it the shift is round(weight), half to even.
        memory_format: torch.contiguous_format (default: a contiguous output) or torch.preserve_format (a dense channels-last
            input comes back channels-last, on HIP tensors interpolated as it lies in one kernel).  A plain attribute, not part
            of the state_dict.
    forward(x) -> output, the tensor alone.  from_float converts a LearnableTemporalShift, active or not, carrying active_flag,
    padding, n_segment and memory_format over.
    """

    def __init__(self, n_segment, in_channels, padding='zeros', active_flag=True, memory_format=torch.contiguous_format):
        super().__init__()
        assert padding.lower() in shifts.paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        assert memory_format in (torch.contiguous_format, torch.preserve_format), \
            f'memory_format must be torch.contiguous_format or torch.preserve_format, not {memory_format}'
        self.memory_format = memory_format
        self.padding = shifts.paddings_dict[padding.lower()]
        self.n_segment = int(n_segment)
        self.in_channels = in_channels
        self._active_flag = bool(active_flag)
        self.register_buffer("weight", torch.zeros(in_channels, 1, dtype=torch.float32))

    def forward(self, input):
        return temporal_shift_learnable_quantized(input, self.weight, self.n_segment, self.padding, self._active_flag, self.memory_format)

    def _get_name(self):
        return 'QuantizedLearnableTemporalShift'

    def extra_repr(self):
        fmt = '' if self.memory_format == torch.contiguous_format else f', memory_format={self.memory_format}'
        return (f'n_segment={self.n_segment}, in_channels={self.in_channels}, padding_method={rp_dict[self.padding]}, '
                f'Active shift on forward pass: {"Yes" if self._active_flag else "No"}' + fmt)

    @classmethod
    def from_float(cls, mod):
        assert isinstance(mod, shifts.LearnableTemporalShift), 'expected a LearnableTemporalShift module'
        qshift = cls(mod.n_segment, mod.in_channels, padding=rp_dict[mod.padding], active_flag=mod._active_flag,
                     memory_format=mod.memory_format)
        qshift.weight = mod.weight.detach().to(torch.float32).reshape(mod.in_channels, 1).clone()
        return qshift


class LearnablePerClipTemporalShift(torch.nn.Module):
    """Quantized per-clip Temporal Shift Module: the float LearnablePerClipTemporalShift / PerClipTemporalShift on per-tensor
    quantized tensors (quint8, qint8, qint32), in the integer domain
    (torchshifts.quantized.functional.temporal_shift_learnable_per_clip_quantized).  Like the float modules it has no parameter and
    no buffer: the table comes from the caller -- a float net that looks at the clip, or per-clip jitter -- and is converted to
    fp32 (detached: the op has no gradient).  The output keeps the input's scale and zero point and is contiguous.

    Arguments:
        n_segment (int): frames per clip, T.
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
        active_flag (bool): interpolate between two frames. Default True; without it the shift is round(table), half to even.
    forward(x, table) -> output, the tensor alone.  table: [N, C], or [N, G] with C % G == 0.  from_float converts a
    LearnablePerClipTemporalShift (its active_flag) or a PerClipTemporalShift (active_flag=False: its integer table).
    """

    def __init__(self, n_segment, padding='zeros', active_flag=True):
        super().__init__()
        assert padding.lower() in shifts.paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        self.padding = shifts.paddings_dict[padding.lower()]
        self.n_segment = int(n_segment)
        self._active_flag = bool(active_flag)

    def forward(self, input, table):
        return temporal_shift_learnable_per_clip_quantized(input, table.detach().to(torch.float32), self.n_segment, self.padding,
                                                           self._active_flag)

    def _get_name(self):
        return 'QuantizedLearnablePerClipTemporalShift'

    def extra_repr(self):
        return (f'n_segment={self.n_segment}, padding_method={rp_dict[self.padding]}, '
                f'Active shift on forward pass: {"Yes" if self._active_flag else "No"}, per-clip weights')

    @classmethod
    def from_float(cls, mod):
        assert isinstance(mod, (shifts.LearnablePerClipTemporalShift, shifts.PerClipTemporalShift)), \
            'expected a LearnablePerClipTemporalShift or a PerClipTemporalShift module'
        active = bool(mod._active_flag) if isinstance(mod, shifts.LearnablePerClipTemporalShift) else False
        return cls(mod.n_segment, padding=rp_dict[mod.padding], active_flag=active)


class TemporalInterlace(torch.nn.Module):
    """Quantized Temporal Interlacing layer (TIN): the float TemporalInterlace on per-tensor quantized tensors (quint8, qint8,
    qint32).  The OffsetNet and the WeightNet stay FLOAT -- they see a [N, fold, T] descriptor, not the activation -- under the
    float module's names, so a float TemporalInterlace checkpoint loads as it is.  The descriptor is formed from the integers: the
    int_repr of the first fold channels summed per (n, t, c) plane in integers, then (sum / M - zero_point) * scale in fp32 -- no
    float tensor of the activation's size is made.  The layer is ONE temporal_interlace_quantized call
    (torchshifts.quantized.functional): the output keeps the input's scale and zero point and is contiguous.  The WeightNet's
    weights lie in (0, 2) and the tensor's scale is kept, so values above half the quantization range saturate (the clamp is part
    of the op's definition): calibrate the activation with that headroom.

    Arguments:
        n_segment (int): frames per clip, T.
        in_channels (int): C.
        shift_div (int): the first C // shift_div channels are interlaced. Default 1 (all of them).
        padding (str): 'zeros' | 'border' | 'periodic' | 'reflect' | 'symmetric'. Default 'zeros'.
    forward(x) -> output, the tensor alone.  from_float converts a TemporalInterlace whose nets are still float: keep them out
    of the conversion with `layer.offset_net.qconfig = layer.weight_net.qconfig = None` before prepare (from_float raises a
    ValueError when convert has already quantized their layers).
    """

    def __init__(self, n_segment, in_channels, shift_div=1, padding='zeros'):
        super().__init__()
        assert padding.lower() in shifts.paddings_dict.keys(), f'incorrect padding option: {padding}'
        assert int(n_segment) >= 1, 'n_segment must be >= 1'
        self.n_segment = int(n_segment)
        self.in_channels = int(in_channels)
        self.shift_div = int(shift_div)
        self.fold = self.in_channels // self.shift_div
        assert self.fold >= 4 and self.fold % 4 == 0, \
            f'in_channels // shift_div ({self.fold}) must be a positive multiple of 4: the fold holds four channel groups'
        self.padding = shifts.paddings_dict[padding.lower()]
        self.offset_net = shifts.OffsetNet(self.fold, self.n_segment)
        self.weight_net = shifts.WeightNet(self.fold)

    def descriptor(self, input):
        """the clip descriptor [N, fold, T] of a quantized input: the dequantized spatial mean of the first fold channels, from an
        integer sum per plane"""
        T, fold = self.n_segment, self.fold
        N = input.shape[0] // T
        q = input[:, :fold].int_repr().reshape(N, T, fold, -1)
        total = q.sum(3, dtype=torch.int64)   # exact
        mean = total.to(torch.float32) / q.shape[3]
        return ((mean - input.q_zero_point()) * input.q_scale()).permute(0, 2, 1)

    def tables(self, input):
        """offsets [N, C] and scales [N, T, C] of the one call (fp32, detached), from the nets' [N, 2] and [N, T, 2]: the float
        module's expansion, the negated offset included"""
        T, C, fold = self.n_segment, self.in_channels, self.fold
        N = input.shape[0] // T
        desc = self.descriptor(input).to(self.offset_net.conv.weight.dtype)
        with torch.no_grad():
            o, w = self.offset_net(desc), self.weight_net(desc)
        table, weight = torch.cat((o, -o), 1), torch.cat((w, w), 2)          # [N, 4], [N, T, 4]
        offsets = (-table).repeat_interleave(fold // 4, dim=1)               # (the op's sign: out[t] = x[t - w])
        scales = weight.repeat_interleave(fold // 4, dim=2)
        if fold < C:
            offsets = torch.cat((offsets, offsets.new_zeros(N, C - fold)), 1)
            scales = torch.cat((scales, scales.new_ones(N, T, C - fold)), 2)
        return offsets.detach().to(torch.float32), scales.detach().to(torch.float32)

    def forward(self, input):
        assert input.shape[1] == self.in_channels and input.shape[0] % self.n_segment == 0, \
            f'expected a [N * {self.n_segment}, {self.in_channels}, ...] tensor, but it is shape is {tuple(input.shape)}'
        offsets, scales = self.tables(input)
        return temporal_interlace_quantized(input, offsets, scales, self.n_segment, self.padding, True)

    def _get_name(self):
        return 'QuantizedTemporalInterlace'

    def extra_repr(self):
        return (f'n_segment={self.n_segment}, in_channels={self.in_channels}, shift_div={self.shift_div}, '
                f'padding_method={rp_dict[self.padding]}')

    @classmethod
    def from_float(cls, mod):
        assert isinstance(mod, shifts.TemporalInterlace), 'expected a TemporalInterlace module'
        layers = ((mod.offset_net.conv, torch.nn.Conv1d), (mod.offset_net.fc1, torch.nn.Linear), (mod.offset_net.fc2, torch.nn.Linear),
                  (mod.weight_net.conv, torch.nn.Conv1d))
        if any(type(layer) is not kind for layer, kind in layers):
            raise ValueError("quantized TemporalInterlace keeps a float OffsetNet / WeightNet, but their layers are no longer float "
                             "nn.Conv1d / nn.Linear: set `layer.offset_net.qconfig = layer.weight_net.qconfig = None` before prepare")
        qmod = cls(mod.n_segment, mod.in_channels, shift_div=mod.shift_div, padding=rp_dict[mod.padding])
        qmod.offset_net = copy.deepcopy(mod.offset_net)
        qmod.weight_net = copy.deepcopy(mod.weight_net)
        return qmod


class OnlineTemporalShift(shifts.OnlineTemporalShift):
    """Quantized online Temporal Shift Module: the float OnlineTemporalShift on per-tensor quantized frames (quint8, qint8, qint32).
    The table is the same persistent int64 buffer `shifts`, so a float checkpoint loads as it is.  The state is a quantized tensor
    with the first frame's scale and zero point -- the zero point in every slot under zeros padding -- and the output keeps the
    frame's scale and zero point; a later frame with other quantization parameters raises.  On HIP tensors the table is passed as
    int32.

    forward(frame) -> the shifted frame alone.  from_float converts an OnlineTemporalShift and carries `inplace` over.
    """

    def _step(self, frame, state, table):
        return (temporal_shift_online_quantized_ if self.inplace else temporal_shift_online_quantized)(frame, state, table)

    def _get_name(self):
        return 'QuantizedOnlineTemporalShift'

    @classmethod
    def from_float(cls, mod):
        assert isinstance(mod, shifts.OnlineTemporalShift), 'expected an OnlineTemporalShift module'
        qshift = cls(mod.in_channels, fold_div=mod.fold_div, shifts=mod.shifts.detach().cpu(), padding=rp_dict[mod.padding],
                     inplace=mod.inplace)
        return qshift.to(mod.shifts.device)
