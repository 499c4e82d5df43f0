from .shifts import GroupedShift1d, GroupedShift2d, GroupedShift3d, LearnablePerClipTemporalShift, LearnableTemporalShift, PerClipTemporalShift, Shift1d, Shift2d, Shift3d, TemporalShift  # noqa: F401
