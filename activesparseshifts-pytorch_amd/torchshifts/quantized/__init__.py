"""torchshifts.quantized: quantized modules + `quant_mapping` for torch.ao.quantization.convert.

The reference builds its mapping tables from torch.quantization internals that no longer exist on
torch >= 2.x (torchshifts/quantized/__init__.py:6-15 raises AttributeError there); this version
looks them up defensively so that importing the package never fails.
"""
import copy

import torch


def _default_static_mappings():
    for modname in ("torch.ao.quantization.quantization_mappings", "torch.quantization.quantization_mappings"):
        try:
            mod = __import__(modname, fromlist=["x"])
            return copy.copy(mod.get_default_static_quant_module_mappings())
        except Exception:  # pragma: no cover - depends on the torch build
            continue
    return {}


tndm_mapping = _default_static_mappings()

from .modules import LearnablePerClipTemporalShift, LearnableTemporalShift, OnlineTemporalShift, Shift1d, Shift2d, Shift3d, TemporalInterlace, TemporalShift, interlacing_quant_mapping, interpolating_quant_mapping, new_quant_mapping  # noqa: E402,F401

quant_mapping = {**tndm_mapping, **new_quant_mapping}
# ... for a net trained with LearnableTemporalShift(active_flag=True): its entry is quantized.LearnableTemporalShift
quant_mapping_interpolating = {**tndm_mapping, **interpolating_quant_mapping}
# ... plus PerClipTemporalShift / LearnablePerClipTemporalShift / TemporalInterlace -> quantized.LearnablePerClipTemporalShift /
# quantized.TemporalInterlace (set offset_net.qconfig = weight_net.qconfig = None on a TemporalInterlace: its nets stay float)
quant_mapping_interlacing = {**tndm_mapping, **interlacing_quant_mapping}
