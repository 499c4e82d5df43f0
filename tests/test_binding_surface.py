"""The surface of the torch operator library (torchshifts:: and the two later namespaces, torchshifts_per_clip:: and
torchshifts_inplace::), pinned on CPU tensors: every schema string, which dispatch keys hold a kernel for every
op, the whole message of every double-backward guard and of every argument refusal a CPU tensor can reach, and what each forward
node saves.  Nothing here computes anything of size: the point is that a change to csrc/torch_binding.cpp that moves a name, a key,
a message or a saved tensor fails a test that says which.

Shapes are the smallest that keep the dimensions apart: N = 2 clips of T = 3 frames, C = 5 channels, 2 x 2 frames; the spatial
families take [2, 5, 4, ...] so that a pool of 2 leaves 2.
"""
import pytest
import torch

import torchshifts  # noqa: F401

OPS = torch.ops.torchshifts
PER_CLIP = torch.ops.torchshifts_per_clip
INPLACE = torch.ops.torchshifts_inplace
N, T, C = 2, 3, 5

SHIFT_FWD = "(Tensor input, Tensor weights, Tensor borders, int[] new_size, int padding_mode, bool active_flag) -> Tensor"
SHIFT_BWD = "(Tensor grad, Tensor weights, Tensor input, Tensor borders, int padding_mode, bool active_flag) -> (Tensor, Tensor)"
POOL_PUB = "(Tensor input, Tensor weights, Tensor borders, int[] pool, int padding_mode, bool active_flag) -> Tensor"
POOL_FWD = "(Tensor input, Tensor weights, Tensor borders, int[] new_size, int[] pool, int padding_mode, bool active_flag) -> Tensor"
POOL_BWD = ("(Tensor grad, Tensor weights, Tensor input, Tensor borders, int[] pool, int padding_mode, bool active_flag)"
            " -> (Tensor, Tensor)")
FIXED_PUB = "(Tensor input, Tensor shifts, Tensor borders, int padding_mode) -> Tensor"
FIXED_BWD = "(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int padding_mode) -> Tensor"
FIXED_POOL_PUB = "(Tensor input, Tensor shifts, Tensor borders, int[] pool, int padding_mode) -> Tensor"
FIXED_POOL_BWD = "(Tensor grad, Tensor shifts, Tensor borders, int[] input_size, int[] pool, int padding_mode) -> Tensor"
TEMPORAL = "(Tensor input, Tensor shifts, int n_segment, int padding_mode) -> Tensor"
TEMPORAL_BWD = "(Tensor grad, Tensor shifts, int n_segment, int padding_mode) -> Tensor"
TSL_FWD = "(Tensor input, Tensor weights, int n_segment, int padding_mode, bool active_flag) -> Tensor"
TSL_BWD = "(Tensor grad, Tensor weights, Tensor input, int n_segment, int padding_mode, bool active_flag) -> (Tensor, Tensor)"
INFERRED = "(Tensor _0, Tensor _1, Tensor _2, int _3, bool _4) -> Tensor _0"

# op -> its argument list and returns, as torch prints them behind "torchshifts::<op>"
SCHEMAS = {
    "_cuda_version": "() -> int _0",
    "_hip_version": "() -> int _0",
    "_check_borders": "(Tensor _0, Tensor _1, int _2) -> (Tensor _0, int[] _1)",
    "shift1d": INFERRED,
    "shift2d": INFERRED,
    "shift3d": INFERRED,
    "_shift1d_forward": SHIFT_FWD,
    "_shift2d_forward": SHIFT_FWD,
    "_shift3d_forward": SHIFT_FWD,
    "_shift1d_backward": SHIFT_BWD,
    "_shift2d_backward": SHIFT_BWD,
    "_shift3d_backward": SHIFT_BWD,
    "shift1d_pool": POOL_PUB,
    "shift2d_pool": POOL_PUB,
    "shift3d_pool": POOL_PUB,
    "_shift1d_pool_forward": POOL_FWD,
    "_shift2d_pool_forward": POOL_FWD,
    "_shift3d_pool_forward": POOL_FWD,
    "_shift1d_pool_backward": POOL_BWD,
    "_shift2d_pool_backward": POOL_BWD,
    "_shift3d_pool_backward": POOL_BWD,
    "shift1d_fixed": FIXED_PUB,
    "shift2d_fixed": FIXED_PUB,
    "shift3d_fixed": FIXED_PUB,
    "_shift1d_fixed_backward": FIXED_BWD,
    "_shift2d_fixed_backward": FIXED_BWD,
    "_shift3d_fixed_backward": FIXED_BWD,
    "shift1d_fixed_pool": FIXED_POOL_PUB,
    "shift2d_fixed_pool": FIXED_POOL_PUB,
    "shift3d_fixed_pool": FIXED_POOL_PUB,
    "_shift1d_fixed_pool_backward": FIXED_POOL_BWD,
    "_shift2d_fixed_pool_backward": FIXED_POOL_BWD,
    "_shift3d_fixed_pool_backward": FIXED_POOL_BWD,
    "temporal_shift": TEMPORAL,
    "_temporal_shift_backward": TEMPORAL_BWD,
    "temporal_shift_quantized": TEMPORAL,
    "temporal_shift_cl": TEMPORAL,
    "_temporal_shift_cl_backward": TEMPORAL_BWD,
    "temporal_shift_quantized_cl": TEMPORAL,
    "temporal_shift_learnable": TSL_FWD,
    "_temporal_shift_learnable_forward": TSL_FWD,
    "_temporal_shift_learnable_backward": TSL_BWD,
    "temporal_shift_learnable_cl": TSL_FWD,
    "_temporal_shift_learnable_cl_forward": TSL_FWD,
    "_temporal_shift_learnable_cl_backward": TSL_BWD,
}

KEYS = ("Autograd", "CPU", "CUDA", "QuantizedCPU", "QuantizedCUDA", "CompositeImplicitAutograd")
COMPOSITE = ("CompositeImplicitAutograd",)
FLOAT = ("Autograd", "CPU", "CUDA")
QUANT = ("QuantizedCPU", "QuantizedCUDA")

# op -> the keys of KEYS that hold a kernel for it
KERNELS = {
    "_cuda_version": COMPOSITE,
    "_hip_version": COMPOSITE,
    "_check_borders": COMPOSITE,
    "shift1d": COMPOSITE,
    "shift2d": COMPOSITE,
    "shift3d": COMPOSITE,
    "_shift1d_forward": FLOAT + QUANT,
    "_shift2d_forward": FLOAT + QUANT,
    "_shift3d_forward": FLOAT + QUANT,
    "_shift1d_backward": FLOAT + QUANT,
    "_shift2d_backward": FLOAT + QUANT,
    "_shift3d_backward": FLOAT + QUANT,
    "shift1d_pool": COMPOSITE,
    "shift2d_pool": COMPOSITE,
    "shift3d_pool": COMPOSITE,
    "_shift1d_pool_forward": FLOAT + ("QuantizedCUDA",),
    "_shift2d_pool_forward": FLOAT + ("QuantizedCUDA",),
    "_shift3d_pool_forward": FLOAT + ("QuantizedCUDA",),
    "_shift1d_pool_backward": FLOAT,
    "_shift2d_pool_backward": FLOAT,
    "_shift3d_pool_backward": FLOAT,
    "shift1d_fixed": COMPOSITE,
    "shift2d_fixed": COMPOSITE,
    "shift3d_fixed": COMPOSITE,
    "_shift1d_fixed_backward": FLOAT,
    "_shift2d_fixed_backward": FLOAT,
    "_shift3d_fixed_backward": FLOAT,
    "shift1d_fixed_pool": COMPOSITE,
    "shift2d_fixed_pool": COMPOSITE,
    "shift3d_fixed_pool": COMPOSITE,
    "_shift1d_fixed_pool_backward": FLOAT,
    "_shift2d_fixed_pool_backward": FLOAT,
    "_shift3d_fixed_pool_backward": FLOAT,
    "temporal_shift": FLOAT,
    "_temporal_shift_backward": FLOAT,
    "temporal_shift_quantized": QUANT,
    "temporal_shift_cl": FLOAT,
    "_temporal_shift_cl_backward": FLOAT,
    "temporal_shift_quantized_cl": QUANT,
    "temporal_shift_learnable": COMPOSITE,
    "_temporal_shift_learnable_forward": FLOAT,
    "_temporal_shift_learnable_backward": FLOAT,
    "temporal_shift_learnable_cl": COMPOSITE,
    "_temporal_shift_learnable_cl_forward": FLOAT,
    "_temporal_shift_learnable_cl_backward": FLOAT,
}


# the two later namespaces: "<namespace>::<op>" -> the same two tables
TEMPORAL_INPLACE = "(Tensor(a!) input, Tensor shifts, int n_segment, int padding_mode) -> Tensor(a!)"
LATER_SCHEMAS = {
    "torchshifts_per_clip::temporal_shift_learnable_per_clip": TSL_FWD,
    "torchshifts_per_clip::_temporal_shift_learnable_per_clip_forward": TSL_FWD,
    "torchshifts_per_clip::_temporal_shift_learnable_per_clip_backward": TSL_BWD,
    "torchshifts_per_clip::temporal_shift_per_clip": TEMPORAL,
    "torchshifts_per_clip::_temporal_shift_per_clip_backward": TEMPORAL_BWD,
    "torchshifts_inplace::temporal_shift_": TEMPORAL_INPLACE,
    "torchshifts_inplace::temporal_shift_quantized_": TEMPORAL_INPLACE,
}
LATER_KERNELS = {
    "torchshifts_per_clip::temporal_shift_learnable_per_clip": COMPOSITE,
    "torchshifts_per_clip::_temporal_shift_learnable_per_clip_forward": FLOAT,
    "torchshifts_per_clip::_temporal_shift_learnable_per_clip_backward": FLOAT,
    "torchshifts_per_clip::temporal_shift_per_clip": FLOAT,
    "torchshifts_per_clip::_temporal_shift_per_clip_backward": FLOAT,
    "torchshifts_inplace::temporal_shift_": FLOAT,
    "torchshifts_inplace::temporal_shift_quantized_": QUANT,
}


def registered_ops(namespace="torchshifts"):
    return sorted(n.split("::", 1)[1] for n in torch._C._dispatch_get_all_op_names() if n.startswith(namespace + "::"))


def test_no_op_beyond_the_pinned_set():
    assert registered_ops() == sorted(SCHEMAS)
    assert sorted(KERNELS) == sorted(SCHEMAS)
    for namespace in ("torchshifts_per_clip", "torchshifts_inplace"):
        assert [namespace + "::" + op for op in registered_ops(namespace)] == sorted(n for n in LATER_SCHEMAS if n.startswith(namespace + "::"))
    assert sorted(LATER_KERNELS) == sorted(LATER_SCHEMAS)


@pytest.mark.parametrize("op", sorted(SCHEMAS))
def test_schema(op):
    assert str(torch._C._get_schema("torchshifts::" + op, "")) == "torchshifts::" + op + SCHEMAS[op]


@pytest.mark.parametrize("op", sorted(KERNELS))
def test_dispatch_keys(op):
    have = tuple(k for k in KEYS if torch._C._dispatch_has_kernel_for_dispatch_key("torchshifts::" + op, k))
    assert have == KERNELS[op]


@pytest.mark.parametrize("op", sorted(LATER_SCHEMAS))
def test_schema_of_the_later_namespaces(op):
    assert str(torch._C._get_schema(op, "")) == op + LATER_SCHEMAS[op]


@pytest.mark.parametrize("op", sorted(LATER_KERNELS))
def test_dispatch_keys_of_the_later_namespaces(op):
    have = tuple(k for k in KEYS if torch._C._dispatch_has_kernel_for_dispatch_key(op, k))
    assert have == LATER_KERNELS[op]


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def message(fn, *args):
    """the whole message of the RuntimeError that fn(*args) raises (what follows a first line is the C++ trace, when one is on)"""
    with pytest.raises(RuntimeError) as e:
        fn(*args)
    return str(e.value).split("\n")[0]


def volume(nd, grad=False):
    return torch.randn((N, C) + (4, 4, 4)[:nd], requires_grad=grad)


def whole(nd):
    """the 6 integers of the window that is the whole [.., 4, ..] volume"""
    return torch.tensor([0, 4 if nd > 0 else 1, 0, 4 if nd > 1 else 1, 0, 4 if nd > 2 else 1], dtype=torch.int32)


def frames(grad=False):
    return torch.randn(N * T, C, 2, 2, requires_grad=grad)


def quantized(t):
    return torch.quantize_per_tensor(t, 0.1, 3, torch.quint8)


# ---- the double-backward guards ------------------------------------------------------------------------------------------------
def grads_of_shift(nd):
    g, w, x = volume(nd, True), torch.randn(C, nd), volume(nd)
    return getattr(OPS, "_shift%dd_backward" % nd)(g, w, x, whole(nd), 0, True), "shift%dd" % nd


def grads_of_pool(nd):
    g, w, x = torch.randn((N, C) + (2,) * nd, requires_grad=True), torch.randn(C, nd), volume(nd)
    return getattr(OPS, "_shift%dd_pool_backward" % nd)(g, w, x, whole(nd), [2] * nd, 0, True), "shift%dd" % nd


def grads_of_fixed(nd):
    g, s = volume(nd, True), torch.ones(C, nd, dtype=torch.int64)
    return getattr(OPS, "_shift%dd_fixed_backward" % nd)(g, s, whole(nd), g.shape, 0), "shift%dd_fixed" % nd


def grads_of_fixed_pool(nd):
    g, s = torch.randn((N, C) + (2,) * nd, requires_grad=True), torch.ones(C, nd, dtype=torch.int64)
    size = (N, C) + (4,) * nd
    return getattr(OPS, "_shift%dd_fixed_pool_backward" % nd)(g, s, whole(nd), size, [2] * nd, 0), "shift%dd_fixed_pool" % nd


def grads_of_temporal(suffix):
    s = torch.tensor([1, 0, -1, 2, 0])
    return getattr(OPS, "_temporal_shift%s_backward" % suffix)(frames(True), s, T, 0), "temporal_shift" + suffix


def grads_of_learnable(suffix):
    w = torch.tensor([0.5, -1.25, 2.0, 0.0, 1.0])
    return (getattr(OPS, "_temporal_shift_learnable%s_backward" % suffix)(frames(True), w, frames(), T, 0, True),
            "temporal_shift_learnable" + suffix)


GUARDED = ([(f, nd) for f in (grads_of_shift, grads_of_pool, grads_of_fixed, grads_of_fixed_pool) for nd in (1, 2, 3)] +
           [(f, s) for f in (grads_of_temporal, grads_of_learnable) for s in ("", "_cl")])


@pytest.mark.parametrize("make,arg", GUARDED, ids=["%s-%s" % (f.__name__[9:], a or "plain") for f, a in GUARDED])
def test_a_second_backward_raises_under_the_ops_name(make, arg):
    out, name = make(arg)
    first = out if torch.is_tensor(out) else out[0]
    assert first.requires_grad
    assert message(first.sum().backward) == "double backwards on %s not supported" % name


def grads_of_per_clip_learnable(_):
    w = torch.randn(N, C)
    return PER_CLIP._temporal_shift_learnable_per_clip_backward(frames(True), w, frames(), T, 0, True), "temporal_shift_learnable_per_clip"


def grads_of_per_clip(_):
    return PER_CLIP._temporal_shift_per_clip_backward(frames(True), torch.ones(N, C, dtype=torch.int64), T, 0), "temporal_shift_per_clip"


@pytest.mark.parametrize("make", [grads_of_per_clip_learnable, grads_of_per_clip], ids=["learnable", "fixed"])
def test_a_second_backward_of_the_per_clip_ops_raises_under_the_ops_name(make):
    out, name = make(None)
    first = out if torch.is_tensor(out) else out[0]
    assert first.requires_grad
    assert message(first.sum().backward) == "double backwards on %s not supported" % name


# ---- argument refusals ---------------------------------------------------------------------------------------------------------
S = torch.tensor([1, 0, -1, 2, 0])                       # a [C] table of shifts
W = torch.tensor([0.5, -1.25, 2.0, 0.0, 1.0])            # [C] learnable shifts
S2 = torch.ones(C, 2, dtype=torch.int64)                 # a [C, 2] table
NONE = torch.Tensor()                                    # "no borders"


def per_channel(t):
    return torch.quantize_per_channel(t, torch.full((C,), 0.1), torch.zeros(C, dtype=torch.int64), 1, torch.quint8)


def segment_refusals(op, prefix, table, kind, extra, wrong_type, types, ops=OPS):
    """the seven lines of a segment family's check, in the order the check has them"""
    call = lambda x, t, n, pad: getattr(ops, op)(x, t, n, pad, *extra)   # noqa: E731
    return [
        (call, (quantized(frames()), table, T, 0), prefix + ": quantized inputs are not supported"),
        (call, (torch.randn(N * T), table, T, 0), prefix + ": expected a [N*T, C, ...] tensor of 2 to 5 dims"),
        (call, (frames(), table, 4, 0), prefix + ": dim 0 (6) must be a multiple of n_segment (4)"),
        (call, (frames(), table[:4], T, 0), prefix + ": %s must have shape [C] or [C, 1]" % kind),
        (call, (frames(), table.to("meta"), T, 0), prefix + ": %s must be on the input's device" % kind),
        (call, (frames(), wrong_type, T, 0), prefix + ": %s must be %s" % (kind, types)),
        (call, (frames(), table, T, 5), prefix + ": padding_mode must be 0..4"),
    ]


def quantized_call(x, s, n, pad):
    return OPS.temporal_shift_quantized(x, s, n, pad)


REFUSALS = (
    # temporal_check, all seven, and the check the two guarded backward ops run before their node
    segment_refusals("temporal_shift", "temporal_shift", S, "shifts", (), S.bool(), "integers or floats") +
    segment_refusals("temporal_shift_cl", "temporal_shift", S, "shifts", (), S.bool(), "integers or floats")[2:4] +
    [(OPS._temporal_shift_backward, (frames(), S, 4, 0), "temporal_shift: dim 0 (6) must be a multiple of n_segment (4)"),
     (OPS._temporal_shift_cl_backward, (frames(), S, T, 7), "temporal_shift: padding_mode must be 0..4")] +
    # temporal_quantized_check
    [(quantized_call, (frames(), quantized(S.float()), T, 0), "temporal_shift_quantized: expected a quantized input"),
     (quantized_call, (per_channel(frames()), S, T, 0), "temporal_shift_quantized: expected a per-tensor quantized input"),
     (quantized_call, (quantized(torch.randn(N * T)), S, T, 0),
      "temporal_shift_quantized: expected a [N*T, C, ...] tensor of 2 to 5 dims"),
     (quantized_call, (quantized(frames()), S, 4, 0), "temporal_shift_quantized: dim 0 (6) must be a multiple of n_segment (4)"),
     (quantized_call, (quantized(frames()), S[:4], T, 0), "temporal_shift_quantized: shifts must have shape [C] or [C, 1]"),
     (quantized_call, (quantized(frames()), quantized(S.float()), T, 0), "temporal_shift_quantized: shifts must be integers or floats"),
     (quantized_call, (quantized(frames()), S.bool(), T, 0), "temporal_shift_quantized: shifts must be integers or floats"),
     (quantized_call, (quantized(frames()), S, T, -1), "temporal_shift_quantized: padding_mode must be 0..4"),
     (OPS.temporal_shift_quantized_cl, (quantized(frames()), S, T, 5), "temporal_shift_quantized: padding_mode must be 0..4")] +
    # tsl_check through the plain ops and the _cl ops (which speak under the plain name), and before the guarded backward nodes
    segment_refusals("temporal_shift_learnable", "temporal_shift_learnable", W, "weights", (True,), S, "floats") +
    segment_refusals("temporal_shift_learnable_cl", "temporal_shift_learnable", W, "weights", (True,), S, "floats") +
    segment_refusals("_temporal_shift_learnable_forward", "temporal_shift_learnable", W, "weights", (True,), S, "floats")[3:4] +
    segment_refusals("_temporal_shift_learnable_cl_forward", "temporal_shift_learnable", W, "weights", (True,), S, "floats")[5:6] +
    [(OPS._temporal_shift_learnable_backward, (frames(), S, frames(), T, 0, True), "temporal_shift_learnable: weights must be floats"),
     (OPS._temporal_shift_learnable_cl_backward, (frames(), W, frames(), 4, 0, True),
      "temporal_shift_learnable: dim 0 (6) must be a multiple of n_segment (4)"),
     (OPS._temporal_shift_learnable_backward, (frames()[:T], W, frames(), T, 0, True),
      "temporal_shift_learnable backward: grad does not match the input")] +
    # check_pool, from the composed CPU kernels and from the fixed op's entry
    [(OPS.shift2d_pool, (volume(2), torch.randn(C, 2), NONE, [2], 0, True), "shift2d_pool: pool must hold 2 window sizes"),
     (OPS.shift1d_pool, (volume(1), torch.randn(C, 1), NONE, [0], 0, True), "shift1d_pool: window sizes must be >= 1"),
     (OPS._shift3d_pool_backward, (torch.randn(N, C, 2, 2, 2), torch.randn(C, 3), volume(3), whole(3), [2, 2], 0, True),
      "shift3d_pool: pool must hold 3 window sizes"),
     (OPS.shift2d_fixed_pool, (volume(2), S2, NONE, [2, 0], 0), "shift2d_pool: window sizes must be >= 1")] +
    # fixed_table
    [(OPS.shift2d_fixed, (volume(2)[0], S2, NONE, 0), "shift2d_fixed: expected a 4-D tensor"),
     (OPS.shift2d_fixed, (volume(2), S2[:, :1], NONE, 0), "shift2d_fixed: shifts must have shape [C, 2]"),
     (OPS.shift3d_fixed_pool, (volume(3), S2, NONE, [2, 2, 2], 0), "shift3d_fixed: shifts must have shape [C, 3]"),
     (OPS.shift2d_fixed, (volume(2), S2.to("meta"), NONE, 0), "shift2d_fixed: shifts must be on the input's device"),
     (OPS.shift1d_fixed, (volume(1), S2[:, :1].bool(), NONE, 0), "shift1d_fixed: shifts must be integers or floats")] +
    # the entries of the fixed ops: quantized inputs (the pooled op says `d_fixed:` too) and the padding mode
    [(OPS.shift2d_fixed, (quantized(volume(2)), S2, NONE, 0),
      "shift2d_fixed: quantized inputs are not supported (the quantized modules already shift by integers)"),
     (OPS.shift2d_fixed_pool, (quantized(volume(2)), S2, NONE, [2, 2], 0),
      "shift2d_fixed: quantized inputs are not supported (the quantized modules already shift by integers)"),
     (OPS.shift2d_fixed, (volume(2), S2, NONE, 5), "shift2d_fixed: padding_mode must be 0..4"),
     (OPS.shift2d_fixed_pool, (volume(2), S2, NONE, [2, 2], 5), "shift2d_fixed_pool: padding_mode must be 0..4")] +
    # borders
    [(OPS.shift2d, (torch.randn(C, 4), torch.randn(C, 2), NONE, 0, True), "shift2d: input has too few dimensions"),
     (OPS.shift2d, (volume(2), torch.randn(C, 2), torch.tensor([1, 1]), 0, True), "borders must hold (left, right) per spatial dim"),
     (OPS._shift2d_pool_backward, (torch.randn(N, C, 2, 2), torch.randn(C, 2), volume(2), whole(2)[:4], [2, 2], 0, True),
      "borders must hold 6 integers [l_i, r_i, l_j, r_j, l_k, r_k]")]
)


SN = torch.ones(N, C, dtype=torch.int64)                 # a [N, C] table of shifts
WN = torch.full((N, C), 0.5)                             # [N, C] learnable shifts


def per_clip_refusals(op, table, kind, extra, wrong_type, types):
    """the seven lines of per_clip_check, in the order the check has them"""
    call = lambda x, t, n, pad: getattr(PER_CLIP, op)(x, t, n, pad, *extra)   # noqa: E731
    prefix = op.lstrip("_").replace("_forward", "")
    return [
        (call, (quantized(frames()), table, T, 0), prefix + ": quantized inputs are not supported"),
        (call, (torch.randn(N * T), table, T, 0), prefix + ": expected a [N*T, C, ...] tensor of 2 to 5 dims"),
        (call, (frames(), table, 4, 0), prefix + ": dim 0 (6) must be a multiple of n_segment (4)"),
        (call, (frames(), table[0], T, 0), prefix + ": %s must have shape [N, C] = [2, 5]" % kind),
        (call, (frames(), table[:1], T, 0), prefix + ": %s must have shape [N, C] = [2, 5]" % kind),
        (call, (frames(), table[:, :4], 2, 0), prefix + ": %s must have shape [N, C] = [3, 5]" % kind),
        (call, (frames(), table.to("meta"), T, 0), prefix + ": %s must be on the input's device" % kind),
        (call, (frames(), wrong_type, T, 0), prefix + ": %s must be %s" % (kind, types)),
        (call, (frames(), table, T, 5), prefix + ": padding_mode must be 0..4"),
    ]


def quantized_inplace(x, s, n, pad):
    return INPLACE.temporal_shift_quantized_(x, s, n, pad)


LATER_REFUSALS = (
    # per_clip_check under both names, and before the guarded backward nodes and the CPU kernels' own lines
    per_clip_refusals("temporal_shift_learnable_per_clip", WN, "weights", (True,), SN, "floats") +
    per_clip_refusals("_temporal_shift_learnable_per_clip_forward", WN, "weights", (True,), SN, "floats")[3:4] +
    per_clip_refusals("temporal_shift_per_clip", SN, "shifts", (), SN.bool(), "integers or floats") +
    [(PER_CLIP._temporal_shift_learnable_per_clip_backward, (frames(), SN, frames(), T, 0, True),
      "temporal_shift_learnable_per_clip: weights must be floats"),
     (PER_CLIP._temporal_shift_learnable_per_clip_backward, (frames()[:T], WN, frames(), T, 0, True),
      "temporal_shift_learnable_per_clip backward: grad does not match the input"),
     (PER_CLIP._temporal_shift_per_clip_backward, (frames(), SN, 4, 0), "temporal_shift_per_clip: dim 0 (6) must be a multiple of n_segment (4)")] +
    # temporal_inplace_check
    segment_refusals("temporal_shift_", "temporal_shift_", S, "shifts", (), S.bool(), "integers or floats", INPLACE) +
    # temporal_quantized_inplace_check
    [(quantized_inplace, (frames(), quantized(S.float()), T, 0), "temporal_shift_quantized_: expected a quantized input"),
     (quantized_inplace, (per_channel(frames()), S, T, 0), "temporal_shift_quantized_: expected a per-tensor quantized input"),
     (quantized_inplace, (quantized(torch.randn(N * T)), S, T, 0), "temporal_shift_quantized_: expected a [N*T, C, ...] tensor of 2 to 5 dims"),
     (quantized_inplace, (quantized(frames()), S, 4, 0), "temporal_shift_quantized_: dim 0 (6) must be a multiple of n_segment (4)"),
     (quantized_inplace, (quantized(frames()), S[:4], T, 0), "temporal_shift_quantized_: shifts must have shape [C] or [C, 1]"),
     # (its device line is out of a CPU tensor's reach, as temporal_shift_quantized's is: a meta table takes the call to another key)
     (quantized_inplace, (quantized(frames()), quantized(S.float()), T, 0), "temporal_shift_quantized_: shifts must be integers or floats"),
     (quantized_inplace, (quantized(frames()), S.bool(), T, 0), "temporal_shift_quantized_: shifts must be integers or floats"),
     (quantized_inplace, (quantized(frames()), S, T, -1), "temporal_shift_quantized_: padding_mode must be 0..4")]
)


@pytest.mark.parametrize("case", range(len(LATER_REFUSALS)),
                         ids=["%02d-%s" % (i, r[2][:48].replace(" ", "_")) for i, r in enumerate(LATER_REFUSALS)])
def test_argument_refusal_of_the_later_namespaces(case):
    fn, args, text = LATER_REFUSALS[case]
    assert message(fn, *args) == text


@pytest.mark.parametrize("case", range(len(REFUSALS)), ids=["%02d-%s" % (i, r[2][:40].replace(" ", "_")) for i, r in enumerate(REFUSALS)])
def test_argument_refusal(case):
    fn, args, text = REFUSALS[case]
    assert message(fn, *args) == text


# ---- what the forward nodes save ---------------------------------------------------------------------------------------------
def saved_shapes(fn):
    seen = []

    def pack(t):
        seen.append(tuple(t.shape))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = fn()
    assert out.requires_grad
    return seen


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_shift_nodes_save_input_weight_and_borders(nd):
    x, w = volume(nd, True), torch.randn(C, nd, requires_grad=True)
    expect = [tuple(x.shape), (C, nd), (6,)]
    assert saved_shapes(lambda: getattr(OPS, "shift%dd" % nd)(x, w, NONE, 0, True)) == expect
    assert saved_shapes(lambda: getattr(OPS, "shift%dd_pool" % nd)(x, w, NONE, [2] * nd, 0, True)) == expect


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_fixed_nodes_save_table_and_borders_never_the_input(nd):
    x, s = volume(nd, True), torch.ones(C, nd, dtype=torch.int64)
    expect = [(C, nd), (6,)]
    assert saved_shapes(lambda: getattr(OPS, "shift%dd_fixed" % nd)(x, s, NONE, 0)) == expect
    assert saved_shapes(lambda: getattr(OPS, "shift%dd_fixed_pool" % nd)(x, s, NONE, [2] * nd, 0)) == expect


@pytest.mark.parametrize("op", ["temporal_shift", "temporal_shift_cl"])
def test_temporal_nodes_save_the_table_alone(op):
    x = frames(True)
    assert saved_shapes(lambda: getattr(OPS, op)(x, S, T, 0)) == [(C,)]
    xc = frames().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    assert saved_shapes(lambda: getattr(OPS, op)(xc, S.reshape(C, 1), T, 0)) == [(C, 1)]


@pytest.mark.parametrize("op", ["temporal_shift_learnable", "temporal_shift_learnable_cl"])
def test_learnable_nodes_save_input_and_weights(op):
    x, w = frames(True), W.clone().requires_grad_(True)
    assert saved_shapes(lambda: getattr(OPS, op)(x, w, T, 0, True)) == [(N * T, C, 2, 2), (C,)]


def test_per_clip_nodes_save_what_the_per_channel_nodes_save():
    x, w = frames(True), WN.clone().requires_grad_(True)
    assert saved_shapes(lambda: PER_CLIP.temporal_shift_learnable_per_clip(x, w, T, 0, True)) == [(N * T, C, 2, 2), (N, C)]
    assert saved_shapes(lambda: PER_CLIP.temporal_shift_per_clip(x, SN, T, 0)) == [(N, C)]


def test_the_inplace_node_saves_the_table_alone():
    assert saved_shapes(lambda: INPLACE.temporal_shift_(frames(True).clone(), S, T, 0)) == [(C,)]
    xc = frames(True).contiguous(memory_format=torch.channels_last)
    assert saved_shapes(lambda: INPLACE.temporal_shift_(xc, S.reshape(C, 1), T, 0)) == [(C, 1)]
