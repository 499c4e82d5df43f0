new_quant_mapping = {}

from .shifts import LearnablePerClipTemporalShift, LearnableTemporalShift, OnlineTemporalShift, Shift1d, Shift2d, Shift3d, TemporalInterlace, TemporalShift  # noqa: E402
import torchshifts.modules.shifts as shifts  # noqa: E402

new_quant_mapping.update({shifts.Shift1d: Shift1d, shifts.Shift2d: Shift2d, shifts.Shift3d: Shift3d,
                          shifts.TemporalShift: TemporalShift, shifts.LearnableTemporalShift: TemporalShift,
                          shifts.OnlineTemporalShift: OnlineTemporalShift})

# quant_mapping with the LearnableTemporalShift entry pointing at the interpolating quantized module (quant_mapping itself keeps the
# frozen one: TemporalShift.from_float refuses an active module rather than round its weights)
interpolating_quant_mapping = {**new_quant_mapping, shifts.LearnableTemporalShift: LearnableTemporalShift}

# ... plus the per-clip modules and the TIN layer pointing at their integer-domain quantized modules (the table, or the nets that
# predict it, stay float)
interlacing_quant_mapping = {**interpolating_quant_mapping, shifts.PerClipTemporalShift: LearnablePerClipTemporalShift,
                             shifts.LearnablePerClipTemporalShift: LearnablePerClipTemporalShift,
                             shifts.TemporalInterlace: TemporalInterlace}
