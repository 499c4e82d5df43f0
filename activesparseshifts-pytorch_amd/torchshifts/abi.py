"""ctypes binding of the C ABI in include/shiftnd_hip.h (libshiftnd_hip.so).

This is the thinnest possible host side: it hands raw device pointers, sizes and strides of torch
tensors to the library.  The dispatcher ops in `_C.so` call exactly the same entry points; tests and
bench.py use this module to reach the kernels without dispatcher/allocator overhead.
"""
import ctypes
import os

import torch

# SHIFTND_HIP_LIB: another build of the library (kernel A/B runs with tools/kbench.py); the dispatcher ops in _C.so
# always use the in-tree library
_LIB_PATH = os.environ.get("SHIFTND_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libshiftnd_hip.so")

F32, F64, F16, BF16, I8, U8, I32 = range(7)
WEIGHTS_F32 = 0x100   # SHIFTND_WEIGHTS_F32: OR-ed onto F16 / BF16 -- fp32 weights (and grad_w) with 16-bit tensors
SHIFT_DIM0 = 0x200    # SHIFTND_SHIFT_DIM0: weights / grad_w are [C]; a 1-D shift along spatial dim 0 of segment-major tensors
#                       (forward, sparse shift, and forward_quantized: of dense channels-last tensors too)
FRAMES = 0x400        # SHIFTND_FRAMES: with SHIFT_DIM0 -- every tensor is dense channels-last (memory order N, S0, S1, S2, C); the
#                       frame kernels serve forward (both modes) and backward, or the call is refused
PER_CLIP = 0x1000     # SHIFTND_PER_CLIP: with SHIFT_DIM0 -- weights / grad_w are [N, C], one row per clip; segment-major tensors, the tshift
#                       kernels, forward (both modes) and backward (0x800 is not assigned)
STREAM = 0x2000       # SHIFTND_STREAM: with SHIFT_DIM0 -- one step of the online temporal shift: sizes {B, C, D, spatial...}, x the state
#                       (read and written, the slot stride in the S0 place), out the frame (read and written), w the [C] table
CLIP_FRAMES = 0x4000  # SHIFTND_CLIP_FRAMES: with SHIFT_DIM0 -- every tensor is dense channels-last as under FRAMES and weights / grad_w are
#                       [N, C] as under PER_CLIP; the frame kernels serve forward (both modes) and backward, or the call is refused
INTERLACE = 0x8000    # SHIFTND_INTERLACE: with SHIFT_DIM0 -- temporal interlacing: the per-clip shift times a scale per (n, t, c) plane; weights /
#                       grad_w are ONE packed array, [N, C] offsets followed by [N, T, C] scales; segment-major tensors, forward (both
#                       modes) and backward
INTERLACE_FRAMES = 0x10000  # SHIFTND_INTERLACE_FRAMES: with SHIFT_DIM0 -- temporal interlacing of dense channels-last tensors (as under
#                       FRAMES) under the packed table of INTERLACE; the frame kernels serve forward (both modes) and backward, or the
#                       call is refused
PATH_NONE, PATH_EMPTY, PATH_PLANE, PATH_STRIDED, PATH_SWEEP, PATH_CL = range(6)

DTYPES = {torch.float32: F32, torch.float64: F64, torch.float16: F16, torch.bfloat16: BF16,
          torch.int8: I8, torch.uint8: U8, torch.int32: I32}

EXPORTS = ["shiftnd_abi_version", "shiftnd_status_string", "shiftnd_last_path", "shiftnd_set_path_policy",
           "shiftnd_set_tuning", "shiftnd_debug_map", "shiftnd_last_kernel",
           "shiftnd_check_borders", "shiftnd_forward", "shiftnd_forward_serves_channels_last", "shiftnd_backward_serves_channels_last",
           "shiftnd_backward_workspace_bytes", "shiftnd_backward",
           "shiftnd_forward_quantized", "shiftnd_pooled_sizes", "shiftnd_backward_pooled_workspace_bytes", "shiftnd_forward_pooled", "shiftnd_backward_pooled", "shiftnd_forward_quantized_pooled", "shiftnd_transpose"]


class Problem(ctypes.Structure):
    _fields_ = [("ndim", ctypes.c_int32), ("dtype", ctypes.c_int32), ("padding_mode", ctypes.c_int32),
                ("active", ctypes.c_int32), ("sizes", ctypes.c_int64 * 5), ("borders", ctypes.c_int32 * 6)]


_lib = None

# Test aid (tests/conftest.py sets it): outputs this module allocates are filled with a byte pattern before the call, so that an
# output element no kernel wrote fails a comparison every time instead of only when the allocator hands back dirty memory.
POISON = False


def _new(shape, like):
    t = torch.empty(list(shape), dtype=like.dtype, device=like.device)
    if POISON and t.numel():
        t.view(-1).view(torch.uint8).fill_(0xA5)
    return t


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(_LIB_PATH)
        i64p = ctypes.POINTER(ctypes.c_int64)
        vp = ctypes.c_void_p
        L.shiftnd_abi_version.restype = ctypes.c_int
        L.shiftnd_status_string.restype = ctypes.c_char_p
        L.shiftnd_status_string.argtypes = [ctypes.c_int]
        L.shiftnd_last_path.restype = ctypes.c_int
        L.shiftnd_last_kernel.restype = ctypes.c_char_p
        L.shiftnd_set_path_policy.argtypes = [ctypes.c_int]
        L.shiftnd_set_tuning.argtypes = [ctypes.c_int, ctypes.c_int]
        L.shiftnd_debug_map.restype = ctypes.c_int
        L.shiftnd_debug_map.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
        L.shiftnd_check_borders.restype = ctypes.c_int
        L.shiftnd_check_borders.argtypes = [i64p, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_int32), i64p]
        L.shiftnd_forward.restype = ctypes.c_int
        L.shiftnd_forward.argtypes = [ctypes.POINTER(Problem), vp, i64p, vp, vp, i64p, vp]
        L.shiftnd_forward_serves_channels_last.restype = ctypes.c_int
        L.shiftnd_forward_serves_channels_last.argtypes = [ctypes.POINTER(Problem), vp, i64p, vp, i64p]
        L.shiftnd_backward_serves_channels_last.restype = ctypes.c_int
        L.shiftnd_backward_serves_channels_last.argtypes = [ctypes.POINTER(Problem), vp, i64p, vp, i64p, vp, i64p]
        L.shiftnd_backward_workspace_bytes.restype = ctypes.c_size_t
        L.shiftnd_backward_workspace_bytes.argtypes = [ctypes.POINTER(Problem)]
        L.shiftnd_backward.restype = ctypes.c_int
        L.shiftnd_backward.argtypes = [ctypes.POINTER(Problem), vp, i64p, vp, i64p, vp, vp, i64p, vp, vp,
                                       ctypes.c_size_t, vp]
        L.shiftnd_forward_quantized.restype = ctypes.c_int
        L.shiftnd_forward_quantized.argtypes = [ctypes.POINTER(Problem), vp, i64p, vp, ctypes.c_int32, ctypes.c_int64,
                                                ctypes.c_int64, vp, i64p, vp]
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.shiftnd_pooled_sizes.restype = ctypes.c_int
        L.shiftnd_pooled_sizes.argtypes = [ctypes.POINTER(Problem), i32p, i64p]
        L.shiftnd_backward_pooled_workspace_bytes.restype = ctypes.c_size_t
        L.shiftnd_backward_pooled_workspace_bytes.argtypes = [ctypes.POINTER(Problem), i32p]
        L.shiftnd_forward_pooled.restype = ctypes.c_int
        L.shiftnd_forward_pooled.argtypes = [ctypes.POINTER(Problem), i32p, vp, vp, vp, vp]
        L.shiftnd_backward_pooled.restype = ctypes.c_int
        L.shiftnd_backward_pooled.argtypes = [ctypes.POINTER(Problem), i32p, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
        L.shiftnd_forward_quantized_pooled.restype = ctypes.c_int
        L.shiftnd_forward_quantized_pooled.argtypes = [ctypes.POINTER(Problem), i32p, vp, vp, ctypes.c_int32, ctypes.c_int64,
                                                       ctypes.c_int64, ctypes.c_int32, vp, vp]
        L.shiftnd_transpose.restype = ctypes.c_int
        L.shiftnd_transpose.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, vp]
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s (%d)" % (what, lib().shiftnd_status_string(rc).decode(), rc))


def strides5(t):
    s = list(t.stride()) + [0] * (5 - t.dim())
    return (ctypes.c_int64 * 5)(*s)


def default_borders(x):
    nd = x.dim() - 2
    b = []
    for d in range(3):
        b += [0, x.shape[2 + d] if d < nd else 1]
    return b


def check_borders(sizes, user, ndim):
    sizes_a = (ctypes.c_int64 * len(sizes))(*sizes)
    out = (ctypes.c_int32 * 6)()
    new = (ctypes.c_int64 * len(sizes))()
    up = None
    if user is not None:
        flat = [int(v) for row in user for v in row]
        up = (ctypes.c_int32 * len(flat))(*flat)
    check(lib().shiftnd_check_borders(sizes_a, len(sizes), up, ndim, out, new), "shiftnd_check_borders")
    shift = 1 if ndim + 1 == len(sizes) else 2
    return list(out), list(new)[:shift + min(ndim, 3)]


def problem(x, pad, active, borders, dtype=None, w=None, shift_dim0=False, frames=False, per_clip=False, stream=False,
            clip_frames=False, interlace=False, interlace_frames=False):
    """w: the weights of the call, if it has float weights -- fp32 weights with an fp16 / bf16 `x` set WEIGHTS_F32 (mixed precision);
    shift_dim0: set SHIFT_DIM0 (the temporal shift: w is [C] and acts on spatial dim 0; x a segment-major view, or, for the
    sparse forward and the quantized forward, a dense channels-last view [N, C, T, M] with strides {T*M*C, 1, M*C, C});
    frames: set FRAMES (with shift_dim0: every tensor is such a dense channels-last view, forward in both modes and backward);
    per_clip: set PER_CLIP (with shift_dim0: w is [N, C], one row per clip, x a segment-major view);
    stream: set STREAM (with shift_dim0: x is the state viewed as [B, C, D, M], see online_views);
    clip_frames: set CLIP_FRAMES (with shift_dim0: w is [N, C], one row per clip, every tensor a dense channels-last view);
    interlace: set INTERLACE (with shift_dim0: w is the packed table -- N * C offsets, then N * T * C scales -- x a segment-major view);
    interlace_frames: set INTERLACE_FRAMES (with shift_dim0: w is that packed table, every tensor a dense channels-last view)"""
    p = Problem()
    p.ndim = x.dim() - 2
    p.dtype = DTYPES[x.dtype] if dtype is None else dtype
    if w is not None and w.dtype == torch.float32 and x.dtype in (torch.float16, torch.bfloat16):
        p.dtype |= WEIGHTS_F32
    if shift_dim0:
        p.dtype |= SHIFT_DIM0
    if frames:
        p.dtype |= FRAMES
    if per_clip:
        p.dtype |= PER_CLIP
    if stream:
        p.dtype |= STREAM
    if clip_frames:
        p.dtype |= CLIP_FRAMES
    if interlace:
        p.dtype |= INTERLACE
    if interlace_frames:
        p.dtype |= INTERLACE_FRAMES
    p.padding_mode = int(pad)
    p.active = int(bool(active))
    for i in range(5):
        p.sizes[i] = x.shape[i] if i < x.dim() else 1
    for i, v in enumerate(default_borders(x) if borders is None else borders):
        p.borders[i] = int(v)
    return p


def out_shape(x, borders):
    nd = x.dim() - 2
    b = default_borders(x) if borders is None else borders
    return list(x.shape[:2]) + [b[2 * d + 1] - b[2 * d] for d in range(nd)]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def forward(x, w, pad, active, borders=None, out=None, shift_dim0=False, frames=False, per_clip=False, clip_frames=False,
            interlace=False, interlace_frames=False):
    """x, w: device tensors (float dtypes; w of x's dtype, or fp32 with an fp16 / bf16 x).  Returns a new contiguous output (or
    fills `out`).  shift_dim0: the flagged call (w [C]; x and out segment-major views, or -- active False -- both dense
    channels-last views, memory order N, S0, S1, S2, C: pass `out`, a new output is contiguous).  frames: with shift_dim0, the
    channels-last call in both modes (pass `out`).  out=x with shift_dim0 (active False): the in-place call, either dense layout.
    per_clip: with shift_dim0, w is [N, C] and x, out are segment-major views.  clip_frames: with shift_dim0, w is [N, C] and x, out
    are dense channels-last views (pass `out`).  interlace: with shift_dim0, w is the packed table (pack_interlace) and x, out are
    segment-major views.  interlace_frames: with shift_dim0, w is the packed table and x, out are dense channels-last views (pass `out`)."""
    p = problem(x, pad, active, borders, w=w, shift_dim0=shift_dim0, frames=frames, per_clip=per_clip, clip_frames=clip_frames,
                interlace=interlace, interlace_frames=interlace_frames)
    if out is None:
        out = _new(out_shape(x, borders), x)
    w = w.contiguous()
    check(lib().shiftnd_forward(ctypes.byref(p), x.data_ptr(), strides5(x), w.data_ptr(), out.data_ptr(), strides5(out),
                                _stream()), "shiftnd_forward")
    return out


def backward_workspace(x, pad, active, borders=None, shift_dim0=False, frames=False, per_clip=False, clip_frames=False,
                       interlace=False, interlace_frames=False):
    p = problem(x, pad, active, borders, shift_dim0=shift_dim0, frames=frames, per_clip=per_clip, clip_frames=clip_frames,
                interlace=interlace, interlace_frames=interlace_frames)
    return torch.empty(int(lib().shiftnd_backward_workspace_bytes(ctypes.byref(p))), dtype=torch.uint8, device=x.device)


def backward(grad_out, w, x, pad, active, borders=None, grad_x=None, grad_w=None, workspace=None, shift_dim0=False, frames=False,
             per_clip=False, clip_frames=False, interlace=False, interlace_frames=False):
    """grad_w comes back in w's dtype (fp32 for fp32 weights with a 16-bit x).  frames: with shift_dim0, grad_out, x and grad_x are
    dense channels-last views (pass `grad_x`).  per_clip: with shift_dim0, w and grad_w are [N, C].  clip_frames: with shift_dim0,
    both: dense channels-last views (pass `grad_x`), w and grad_w [N, C].  interlace: with shift_dim0, w and grad_w are packed tables
    (pack_interlace / unpack_interlace).  interlace_frames: with shift_dim0, the packed tables with dense channels-last views (pass
    `grad_x`)"""
    p = problem(x, pad, active, borders, w=w, shift_dim0=shift_dim0, frames=frames, per_clip=per_clip, clip_frames=clip_frames,
                interlace=interlace, interlace_frames=interlace_frames)
    w = w.contiguous()
    if grad_x is None:
        grad_x = _new(x.shape, x)
    if grad_w is None:
        grad_w = _new(w.shape, w)
    if workspace is None:
        workspace = backward_workspace(x, pad, active, borders, shift_dim0, frames, per_clip, clip_frames, interlace, interlace_frames)
    check(lib().shiftnd_backward(ctypes.byref(p), grad_out.data_ptr(), strides5(grad_out), x.data_ptr(), strides5(x),
                                 w.data_ptr(), grad_x.data_ptr(), strides5(grad_x), grad_w.data_ptr(),
                                 workspace.data_ptr(), workspace.numel(), _stream()), "shiftnd_backward")
    return grad_x, grad_w


def pack_interlace(offsets, scales):
    """the ONE table of an INTERLACE call: the [N, C] offsets immediately followed by the [N, T, C] scales (same dtype)"""
    assert offsets.dtype == scales.dtype and offsets.dim() == 2 and scales.dim() == 3
    return torch.cat([offsets.reshape(-1), scales.reshape(-1)])


def unpack_interlace(table, N, T, C):
    """... and back: views [N, C] and [N, T, C] of a packed table or packed gradient"""
    return table[:N * C].view(N, C), table[N * C:].view(N, T, C)


def backward_input(grad_out, w, input_shape, pad, borders=None, grad_x=None, workspace=None):
    """Input gradient only of the sparse shift: shiftnd_backward with x == NULL and grad_w == NULL (no read of the input, no weight
    gradient).  grad_out: device tensor of the window's sizes; w: [C, nd] float table of grad_out's dtype; input_shape: the
    input's sizes; borders: the 6 absolute ints of check_borders (None = the whole input).  Returns grad_x (new, contiguous)."""
    like = torch.empty(list(input_shape), dtype=grad_out.dtype, device="meta")
    p = problem(like, pad, False, borders)
    w = w.contiguous()
    if grad_x is None:
        grad_x = _new(input_shape, grad_out)
    if workspace is None:   # the negated table of the whole-input window (include/shiftnd_hip.h); a cut window needs none
        workspace = torch.empty(w.numel() * w.element_size(), dtype=torch.uint8, device=grad_out.device)
    check(lib().shiftnd_backward(ctypes.byref(p), grad_out.data_ptr(), strides5(grad_out), None, None, w.data_ptr(),
                                 grad_x.data_ptr(), strides5(grad_x), None, workspace.data_ptr() if workspace.numel() else None,
                                 workspace.numel(), _stream()), "shiftnd_backward (input gradient only)")
    return grad_x


def forward_quantized(xq, wq, w_zero_point, x_zero_point, pad, borders=None, out=None, shift_dim0=False, active=False, frames=False,
                      per_clip=False, interlace=False):
    """xq: int8/uint8/int32 device tensor (int_repr); wq: int8/uint8/int32 device tensor [C, nd].  shift_dim0: the flagged call
    (wq [C]; xq and `out` dense channels-last views, memory order N, S0, S1, S2, C; out=xq: the in-place call, which also takes
    the segment-major layout).  active: p->active -- with shift_dim0 and an fp32 [C] table `wq` (w_zero_point 0) the quantized
    interpolating temporal shift of segment-major views xq and `out`; frames: set FRAMES beside it -- the same call on dense
    channels-last views xq and `out` (strides {T*M*C, 1, M*C, C}).  per_clip / interlace: set PER_CLIP / INTERLACE beside shift_dim0 --
    with an fp32 `wq` (w_zero_point 0) the quantized per-clip temporal shift (wq [N, C]) / quantized temporal interlacing (wq the
    packed table, pack_interlace) of segment-major views xq and `out`, `active` 0 or 1."""
    p = problem(xq, pad, active, borders, shift_dim0=shift_dim0, frames=frames, per_clip=per_clip, interlace=interlace)
    if out is None:
        out = _new(out_shape(xq, borders), xq)
    wq = wq.contiguous()
    check(lib().shiftnd_forward_quantized(ctypes.byref(p), xq.data_ptr(), strides5(xq), wq.data_ptr(), DTYPES[wq.dtype],
                                          int(w_zero_point), int(x_zero_point), out.data_ptr(), strides5(out), _stream()),
          "shiftnd_forward_quantized")
    return out


def online_views(frame, state):
    """the [B, C, D, M] problem view of a state [D, B, C, *spatial] and the [B, C, 1, M] view of its frame [B, C, *spatial], both
    dense in one layout (contiguous, or channels-last: unit channel stride)"""
    B, C = frame.shape[:2]
    M = frame[0, 0].numel()
    D = state.shape[0]
    if frame.is_contiguous():
        return state.view(D, B, C, M).permute(1, 2, 0, 3), frame.view(B, C, 1, M)
    order = [0] + list(range(2, frame.dim())) + [1]   # memory order B, spatial, C
    f = frame.permute(order).reshape(B, 1, M, C).permute(0, 3, 1, 2)
    s = state.permute([0] + [1 + d for d in order]).reshape(D, B, M, C).permute(1, 3, 0, 2)
    assert f.data_ptr() == frame.data_ptr() and s.data_ptr() == state.data_ptr()
    return s, f


def online_step(frame, state, w, w_zero_point=0, pad=0):
    """One step of the online temporal shift in place on `frame` [B, C, *spatial] and `state` [D, B, C, *spatial] (device tensors,
    dense in one layout): the flagged call on their problem views.  w: the [C] table -- x's dtype, or fp32 with an fp16 / bf16
    frame; an int8 / uint8 / int32 table with an int8 / uint8 / int32 frame (the quantized entry point)."""
    s, f = online_views(frame, state)
    p = problem(s, pad, False, None, w=w if w.is_floating_point() else None, shift_dim0=True, stream=True)
    w = w.contiguous()
    if w.is_floating_point():
        check(lib().shiftnd_forward(ctypes.byref(p), s.data_ptr(), strides5(s), w.data_ptr(), f.data_ptr(), strides5(f), _stream()),
              "shiftnd_forward (online)")
    else:
        check(lib().shiftnd_forward_quantized(ctypes.byref(p), s.data_ptr(), strides5(s), w.data_ptr(), DTYPES[w.dtype], int(w_zero_point),
                                              0, f.data_ptr(), strides5(f), _stream()), "shiftnd_forward_quantized (online)")
    return frame


def _pool_arg(pool, nd):
    pool = [int(pool)] * nd if isinstance(pool, int) else [int(k) for k in pool]
    assert len(pool) == nd
    return (ctypes.c_int32 * nd)(*pool)


def pooled_shape(x, pool, borders=None):
    p = problem(x, 0, False, borders)
    sp = (ctypes.c_int64 * 3)()
    check(lib().shiftnd_pooled_sizes(ctypes.byref(p), _pool_arg(pool, p.ndim), sp), "shiftnd_pooled_sizes")
    return list(x.shape[:2]) + list(sp)[:p.ndim]


def forward_pooled(x, w, pad, active, pool, borders=None, out=None):
    """Fused shift + avg_pool(kernel = stride = pool, ceil_mode=True); x, w contiguous device tensors."""
    assert x.is_contiguous()
    p = problem(x, pad, active, borders, w=w)
    if out is None:
        out = _new(pooled_shape(x, pool, borders), x)
    w = w.contiguous()
    check(lib().shiftnd_forward_pooled(ctypes.byref(p), _pool_arg(pool, p.ndim), x.data_ptr(), w.data_ptr(),
                                       out.data_ptr(), _stream()), "shiftnd_forward_pooled")
    return out


REQUANT_ZP_INSIDE, REQUANT_ZP_OUTSIDE = 0, 1


def forward_quantized_pooled(xq, wq, w_zero_point, x_zero_point, pad, pool, borders=None, out=None, requant=REQUANT_ZP_INSIDE):
    """Quantized shift + avg_pool(kernel = stride = pool, ceil_mode=True) in one pass; xq: int8 / uint8 contiguous device
    tensor (int_repr), wq: integer tensor [C, nd]; requant: which of ATen's two roundings (include/shiftnd_hip.h)."""
    assert xq.is_contiguous()
    p = problem(xq, pad, False, borders)
    if out is None:
        out = _new(pooled_shape(xq, pool, borders), xq)
    wq = wq.contiguous()
    check(lib().shiftnd_forward_quantized_pooled(ctypes.byref(p), _pool_arg(pool, p.ndim), xq.data_ptr(), wq.data_ptr(),
                                                 DTYPES[wq.dtype], int(w_zero_point), int(x_zero_point), int(requant), out.data_ptr(),
                                                 _stream()), "shiftnd_forward_quantized_pooled")
    return out


def backward_pooled_workspace_bytes(x, pad, active, pool, borders=None):
    p = problem(x, pad, active, borders)
    return int(lib().shiftnd_backward_pooled_workspace_bytes(ctypes.byref(p), _pool_arg(pool, p.ndim)))


def backward_pooled(grad_pooled, w, x, pad, active, pool, borders=None, grad_x=None, grad_w=None, workspace=None):
    assert x.is_contiguous() and grad_pooled.is_contiguous()
    p = problem(x, pad, active, borders, w=w)
    w = w.contiguous()
    if grad_x is None:
        grad_x = _new(x.shape, x)
    if grad_w is None:
        grad_w = _new(w.shape, w)
    if workspace is None:
        nbytes = int(lib().shiftnd_backward_pooled_workspace_bytes(ctypes.byref(p), _pool_arg(pool, p.ndim)))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    check(lib().shiftnd_backward_pooled(ctypes.byref(p), _pool_arg(pool, p.ndim), grad_pooled.data_ptr(), x.data_ptr(),
                                        w.data_ptr(), grad_x.data_ptr(), grad_w.data_ptr(), workspace.data_ptr(),
                                        workspace.numel(), _stream()), "shiftnd_backward_pooled")
    return grad_x, grad_w


def backward_pooled_input(grad_pooled, w, input_shape, pad, pool, borders=None, grad_x=None):
    """Input gradient only of the sparse shift + average pool: shiftnd_backward_pooled with x == NULL and grad_w == NULL (no read
    of the input, no weight gradient, no workspace).  grad_pooled: contiguous device tensor of the pooled sizes; w: [C, nd] float
    table of its dtype; input_shape: the input's sizes; borders: the 6 absolute ints of check_borders (None = the whole input).
    Returns grad_x (new, contiguous)."""
    assert grad_pooled.is_contiguous()
    like = torch.empty(list(input_shape), dtype=grad_pooled.dtype, device="meta")
    p = problem(like, pad, False, borders)
    w = w.contiguous()
    if grad_x is None:
        grad_x = _new(input_shape, grad_pooled)
    check(lib().shiftnd_backward_pooled(ctypes.byref(p), _pool_arg(pool, p.ndim), grad_pooled.data_ptr(), None, w.data_ptr(),
                                        grad_x.data_ptr(), None, None, 0, _stream()), "shiftnd_backward_pooled (input gradient only)")
    return grad_x


def to_contiguous(x, out=None):
    """channels-last dense [N, C, spatial...] device tensor -> new contiguous tensor (shiftnd_transpose), or fills the contiguous `out`"""
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous()
    P = x[0, 0].numel()
    check(lib().shiftnd_transpose(x.data_ptr(), out.data_ptr(), x.shape[0], P, x.shape[1], x.element_size(), _stream()),
          "shiftnd_transpose")
    return out


def to_channels_last(x, out=None):
    """contiguous [N, C, spatial...] device tensor -> new channels-last dense tensor (shiftnd_transpose), or fills the
    channels-last dense `out`"""
    fmt = torch.channels_last if x.dim() == 4 else torch.channels_last_3d
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device, memory_format=fmt)
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous(memory_format=fmt)
    P = x[0, 0].numel()
    check(lib().shiftnd_transpose(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], P, x.element_size(), _stream()),
          "shiftnd_transpose")
    return out


def last_path():
    return lib().shiftnd_last_path()


def last_kernel():
    return lib().shiftnd_last_kernel().decode()


def set_path_policy(policy):
    lib().shiftnd_set_path_policy(int(policy))


def set_tuning(knob, value):
    """diagnostics: launch-planning knobs (see include/shiftnd_hip.h)"""
    lib().shiftnd_set_tuning(int(knob), int(value))
