"""Case table, data generator and reference of the big-index tests: one call on one tensor past 2^31 elements / 4 GiB, compared whole
(tests/test_bigindex_gpu.py on the GPU, tests/test_bigindex_cases.py for the self-checks that need none).

REFERENCE.  Plain torch on whatever device its inputs are on: index arithmetic in int64, values in fp64.  It restates the oracle
(oracle/shift_oracle.c) -- the padding map, the corner order, the blend order, the weight preparation of forward and backward, the
weight-gradient expressions as the reference wires them -- for 1 to 3 shifted dims with any trailing dims riding along, the whole window
or a cut one, and the quantized gather with its zero-point fill.  The temporal shift is the 1-D problem on the view [N, C, T, ...];
the fused 2 x 2 average pool is the module's two-step sequence.  No op here couples samples, so the reference of a slice of samples
(clips) is the slice of the reference: the GPU tests hand it chunks whose indices start at zero while the kernel saw the big ones.

DATA.  The project's exact data (pooled16_cases.exact_data): x and gradients are multiples of 1/8 with |k| <= 7, the weights lie on
quarters (halves in 3-D) and are narrowed to bf16.  Every tap, every blend and grad_x is then exact in fp32 and representable in fp16
and bf16: a correct kernel returns the fp64 reference, narrowed, bit for bit.  x is drawn from [0, 7/8] in the big cases (the
full-size fixture's offset: tests/test_fullsize_properties.py draws x from [0, 1)).  Chunks of samples are drawn on the device from a
generator seeded with (seed, chunk): the test writes them into the big tensor and draws them again for the reference, so no second
copy of the tensor exists.
"""
import numpy as np
import torch

F16, BF16, F32, F64, U8, I8, I32 = torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int8, torch.int32
DTYPES = {"f16": F16, "bf16": BF16, "f32": F32, "u8": U8}
CHUNK_BYTES = 64 << 20      # of the tensor's own type per chunk of samples (the fp64 temporaries are 4 to 8 times that)
EL30, EL31, EL32, BYTE32 = "2^30 elements", "2^31 elements", "2^32 elements", "2^32 bytes"
MARKS = {EL30: 1 << 30, EL31: 1 << 31, EL32: 1 << 32}


def es_of(dt):
    return torch.empty(0, dtype=dt).element_size()


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def fold(idx, L, pad):
    """oracle_infer_index on an int64 tensor -> (index inside [0, L), valid): zeros padding marks what lies outside"""
    ones = torch.ones_like(idx, dtype=torch.bool)
    if L == 1:                                       # (gather_offset: a dim of size 1 reads its only element)
        return torch.zeros_like(idx), ones
    if pad == 0:
        return idx.clamp(0, L - 1), (idx >= 0) & (idx <= L - 1)
    if pad == 1:
        return idx.clamp(0, L - 1), ones
    if pad == 2:
        return torch.remainder(idx, L), ones
    period = L - 1 if pad == 3 else L
    neg = (idx < 0).to(torch.int64)
    odd = (neg + torch.div(idx.abs() - neg, period, rounding_mode="floor")) & 1
    m = torch.remainder(idx, period)
    return torch.where(odd.bool(), L - 1 - m, m), ones


def _prep_forward(w64, active):
    iw = torch.floor(w64) if active else torch.round(w64)          # (torch.round: half to even, as rint)
    return iw.to(torch.int64), (w64 - iw if active else torch.zeros_like(w64))


def _prep_backward(w64, active):
    fl = torch.floor(w64)
    if active:
        d = w64 - fl
        return (w64 - d).to(torch.int64), d
    d = torch.where(w64 > 0, w64 - fl, torch.ceil(w64) - w64)
    return torch.round(w64).to(torch.int64), d


def _windows(sizes, nd, borders):
    if borders is None:
        return [(0, int(sizes[d])) for d in range(nd)]
    return [(int(borders[2 * d]), int(borders[2 * d + 1])) for d in range(nd)]


def _per_channel(v, C, nd, trailing):
    """[C] -> [1, C, 1 ...] against [n, C, nd dims, trailing dims]"""
    return v.view([1, C] + [1] * (nd + trailing))


def _gather(t, idx, valid, nd):
    """t [n, C, S_0 .. S_nd-1, trailing ...]; idx, valid: per dim [C, O_d] -> t at (c, idx_0[c, .], idx_1[c, .] ...) of shape
    [n, C, O_0 .. O_nd-1, trailing ...] and the mask [1, C, O ..., 1 ...] of the positions every dim accepts"""
    C = t.shape[1]
    trailing = t.dim() - 2 - nd

    def shaped(a, d):
        return a.view([C] + [a.shape[1] if e == d else 1 for e in range(nd)])

    ci = torch.arange(C, device=t.device).view([C] + [1] * nd)
    v = t[(slice(None), ci) + tuple(shaped(idx[d], d) for d in range(nd))]
    ok = shaped(valid[0], 0)
    for d in range(1, nd):
        ok = ok & shaped(valid[d], d)
    return v, ok.view([1] + list(ok.shape) + [1] * trailing)


def _i1(a, b, t):
    return a * (1 - t) + b * t                                     # interp1D, in the oracle's order


def _blend(vals, d):
    """interp1D / 2D / 3D: corner q has bit e set for +1 along dim e; dim 0 is blended first"""
    for t in d:
        vals = [_i1(vals[2 * k], vals[2 * k + 1], t) for k in range(len(vals) // 2)]
    return vals[0]


def shift_forward(x, w, pad, active, nd, borders=None, fill=None):
    """x [n, C, S_0 .. S_nd-1, trailing ...]; w [C, nd].  Floats: -> fp64 of the window's shape.  fill given: the quantized gather --
    w holds the integer shifts, the result keeps x's type and `fill` stands where zeros padding reads nothing"""
    C, S = x.shape[1], x.shape[2:2 + nd]
    trailing = x.dim() - 2 - nd
    win = _windows(S, nd, borders)
    if fill is not None:
        iw, active = w.to(torch.int64), False
    else:
        iw, dw = _prep_forward(w.to(F64), active)
    base = [torch.arange(l, r, device=x.device).view(1, -1) - iw[:, d:d + 1] for d, (l, r) in enumerate(win)]
    vals = []
    for q in range(2 ** nd if active else 1):
        folded = [fold(base[d] + ((q >> d) & 1), int(S[d]), pad) for d in range(nd)]
        v, ok = _gather(x, [f[0] for f in folded], [f[1] for f in folded], nd)
        if fill is not None:
            return torch.where(ok, v, torch.full((), fill, dtype=x.dtype, device=x.device))
        vals.append(torch.where(ok, v, torch.zeros((), dtype=x.dtype, device=x.device)).to(F64))
    if not active:
        return vals[0]
    return _blend(vals, [_per_channel(dw[:, d], C, nd, trailing) for d in range(nd)])


def shift_backward(go, x, w, pad, active, nd, borders=None, sizes=None):
    """go: the window's shape; x as in shift_forward -> grad_x (fp64, x's shape), grad_w (fp64 [C, nd]: the sum over THESE samples).
    x None: the input gradient alone (`sizes`: the input's shifted dims) -> grad_x, None"""
    C, S = go.shape[1], (sizes if x is None else x.shape[2:2 + nd])
    trailing = go.dim() - 2 - nd
    win = _windows(S, nd, borders)
    O = [r - l for l, r in win]
    cropped = any(o != int(s) for o, s in zip(O, S))
    iw, dw = _prep_backward(w.to(F64), active)
    d = [_per_channel(dw[:, e], C, nd, trailing) for e in range(nd)]
    pos = [torch.arange(int(S[e]), device=go.device) for e in range(nd)]
    inside = [((pos[e] >= win[e][0]) & (pos[e] < win[e][1])).view(1, -1).expand(C, -1) for e in range(nd)]
    gw = None
    if x is not None:
        gw = _weight_gradient(go, x, pad, nd, win, cropped, iw, d, pos, inside)
    # grad_x: the window read at oi - shift (+ corner) and blended (interpolating), or at oi + shift (sparse)
    oi = [pos[e].view(1, -1) - win[e][0] for e in range(nd)]
    vals = []
    for q in range(2 ** nd if active else 1):
        if active:
            folded = [fold(oi[e] - iw[:, e:e + 1] + ((q >> e) & 1), O[e], pad) for e in range(nd)]
        else:
            folded = [fold(oi[e] + iw[:, e:e + 1], O[e], pad) for e in range(nd)]
        g, ok = _gather(go, [f[0] for f in folded], [f[1] & inside[e] for e, f in enumerate(folded)], nd)
        vals.append(torch.where(ok, g, torch.zeros((), dtype=go.dtype, device=go.device)).to(F64))
    return (_blend(vals, d) if active else vals[0]), gw


def _weight_gradient(go, x, pad, nd, win, cropped, iw, d, pos, inside):
    S = x.shape[2:2 + nd]
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    # the corners of x around every input position (all 2^nd of them, whatever the mode), zero outside the window
    v = []
    for q in range(2 ** nd):
        folded = [fold(pos[e].view(1, -1) - iw[:, e:e + 1] + ((q >> e) & 1), int(S[e]), pad) for e in range(nd)]
        g, ok = _gather(x, [f[0] for f in folded], [f[1] & inside[e] for e, f in enumerate(folded)], nd)
        v.append(torch.where(ok, g, zero).to(F64))
    if nd == 1:
        wg = [v[1] - v[0]]
    elif nd == 2:      # (interp2D_dx / _dy as the reference calls them: both differences run along dim 1)
        wg = [_i1(v[2] - v[0], v[3] - v[1], d[1]), _i1(v[2], v[3], d[0]) - _i1(v[0], v[1], d[0])]
    else:
        def dx2(a, y):
            return _i1(a[2] - a[0], a[3] - a[1], y)

        def dy2(a, t):
            return _i1(a[2], a[3], t) - _i1(a[0], a[1], t)

        def i2(a):
            return _i1(_i1(a[0], a[1], d[0]), _i1(a[2], a[3], d[0]), d[1])

        wg = [_i1(dx2(v[:4], d[1]), dx2(v[4:], d[1]), d[2]), _i1(dy2(v[:4], d[0]), dy2(v[4:], d[0]), d[2]), i2(v[4:]) - i2(v[:4])]
    del v
    go64 = go.to(F64)
    if cropped:
        full = torch.zeros(x.shape, dtype=F64, device=x.device)
        full[(slice(None), slice(None)) + tuple(slice(l, r) for l, r in win)] = go64
    else:
        full = go64
    sum_dims = [0] + list(range(2, x.dim()))
    return torch.stack([(full * t).sum(dim=sum_dims) for t in wg], dim=1)


def temporal_forward(x, w, pad, active):
    """x: the view [n, C, T, ...] of the clips (any strides); w [C]"""
    return shift_forward(x, w.reshape(-1, 1), pad, active, 1)


def temporal_backward(go, x, w, pad, active):
    gx, gw = shift_backward(go, x, w.reshape(-1, 1), pad, active, 1, sizes=go.shape[2:3])
    return gx, (None if gw is None else gw.reshape(-1))


def temporal_forward_q(xq, shifts, fill, pad):
    return shift_forward(xq, shifts.reshape(-1, 1), pad, False, 1, fill=fill)


def narrow(t64, dt):
    """fp64 -> fp32 -> the storage type, as the kernels narrow (the identity on exact data)"""
    return t64.to(F32).to(dt)


def avg_pool2(y64):
    """2 x 2 windows over the last two dims, both even: every window holds four elements"""
    n = list(y64.shape)
    assert n[-1] % 2 == 0 and n[-2] % 2 == 0
    return y64.reshape(n[:-2] + [n[-2] // 2, 2, n[-1] // 2, 2]).sum(dim=(-3, -1)) / 4


def avg_pool2_backward(gp64):
    return (gp64 / 4).repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


def pooled_forward(x, w, pad, active, dt):
    """the module's two steps: the shift narrowed to the storage type, then the pool narrowed once"""
    return narrow(avg_pool2(narrow(shift_forward(x, w, pad, active, 2), dt).to(F64)), dt)


def pooled_backward(gp, x, w, pad, active, dt):
    g = narrow(avg_pool2_backward(gp.to(F64)), dt)
    return shift_backward(g, x, w, pad, active, 2, sizes=g.shape[2:4])


def pooled_forward_q(xq, shifts, zp, pad, inside=True):
    """the quantized gather, then ATen's quantized average pool over windows of four: nearbyint(zp + sum(x - zp) / 4) (the zero point
    inside the rounding) or nearbyint(sum / 4) + zp, clamped to the type"""
    y = shift_forward(xq, shifts, pad, False, 2, fill=zp).to(F64) - zp
    s = avg_pool2(y)
    q = torch.round(zp + s) if inside else torch.round(s) + zp
    info = torch.iinfo(xq.dtype)
    return q.clamp(info.min, info.max).to(xq.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def eighths(seed, chunk, shape, dt, device, lo=-7, hi=7):
    """multiples of 1/8, k in [lo, hi], drawn on `device` from (seed, chunk) -- the same values every time they are asked for"""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) * 1000003 + int(chunk))
    k = torch.randint(lo, hi + 1, tuple(shape), generator=g, device=device, dtype=torch.int8)
    return (k.to(F32) / 8).to(dt)


def bytes_(seed, chunk, shape, dt, device):
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) * 1000003 + int(chunk))
    info = torch.iinfo(dt)
    return torch.randint(info.min, info.max + 1, tuple(shape), generator=g, device=device, dtype=torch.int16).to(dt)


def draw(seed, chunk, shape, dt, device, lo=-7, hi=7):
    return bytes_(seed, chunk, shape, dt, device) if dt in (U8, I8) else eighths(seed, chunk, shape, dt, device, lo, hi)


def spatial_weights(C, sizes, seed):
    """[C, nd] fp32 on quarters (halves in 3-D), bf16-representable.  Channels 0-3: 0 / beyond the dim / minus half the dim / ties of
    the sparse shift's rounding; the rest drawn in [-3.5, 3.5], so neighbouring channels differ"""
    nd = len(sizes)
    grid = 4.0 if nd <= 2 else 2.0
    rs = np.random.RandomState(seed)
    w = rs.randint(-int(3.5 * grid), int(3.5 * grid) + 1, size=(C, nd)) / grid
    s = np.array(sizes, np.float64)
    for c, row in enumerate([np.zeros(nd), s + 1 + 1 / grid, -s / 2, np.array([0.5, -2.5, 2.5][:nd])][:C]):
        w[c] = row
    w = torch.from_numpy(w).to(BF16).to(F32)
    assert torch.equal(w * grid, torch.round(w * grid))
    assert bool((w[1].abs() > torch.tensor(s)).all()) if C > 1 else True
    return w


def spatial_shifts(C, sizes, seed):
    """[C, nd] int64 for the quantized gather: 0 / beyond the dim / negative / neighbours that differ"""
    nd = len(sizes)
    rs = np.random.RandomState(seed)
    s = rs.randint(-3, 4, size=(C, nd))
    for c, row in enumerate([[0] * nd, [v + 3 for v in sizes], [-(v // 2) for v in sizes], [1, -1, 2][:nd]][:C]):
        s[c] = row
    return torch.from_numpy(s.astype(np.int64))


def temporal_weights(C, T, seed):
    """[C] fp32 on quarters in [-(T + 1), T + 1]; channels 0-5: 0, 2, T + 1, -(T + 1), 0.5, -0.25 (tests/test_tshift_gpu.py)"""
    rs = np.random.RandomState(seed)
    w = rs.randint(-4 * (T + 1), 4 * (T + 1) + 1, size=C) / 4.0
    for c, v in enumerate([0.0, 2.0, T + 1.0, -(T + 1.0), 0.5, -0.25][:C]):
        w[c] = v
    w = torch.from_numpy(w).to(BF16).to(F32)
    assert torch.equal(w * 4, torch.round(w * 4))
    return w


def temporal_shifts(C, T, seed):
    """[C] int64: channels 0-15 drawn in [-(T + 1), T + 1] behind 0, T + 1, -(T + 1), -1 (pieces whose channels differ: the
    element-by-element path of frames_forward), then runs of 8 channels (-1, 1, 0, T + 1, -(T + 1), 2: whole pieces with one source)"""
    rs = np.random.RandomState(seed)
    s = rs.randint(-T - 1, T + 2, size=C)
    for c, v in enumerate([0, T + 1, -(T + 1), -1][:C]):
        s[c] = v
    runs = (-1, 1, 0, T + 1, -(T + 1), 2)
    for c in range(16, C):
        s[c] = runs[((c - 16) // 8) % len(runs)]
    return torch.from_numpy(s.astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the limits, copied as arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def segment_limit_ok(N, T, C, inner, es):
    """segment_forward_eligible (csrc/shiftnd_segment.hip): planes * units per plane + 16 < 2^31; the unit is the element where it
    is one byte, two bytes elsewhere"""
    limit = 1 << 31
    if T >= (1 << 30) or inner >= limit or N >= limit or C >= limit or N * T >= limit:
        return False
    planes = N * T * C
    return planes < limit and planes * (inner if es == 1 else inner * es // 2) + 16 < limit


def tshift_limit_ok(N, T, C, inner, es):
    """tshift_geometry_ok (csrc/shiftnd_tshift.hip; include/shiftnd_hip.h: "fewer than 2^31 - 16 two-byte units in the tensor")"""
    limit = 1 << 31
    if T >= (1 << 30) or inner >= limit or N >= limit or C >= limit or N * T >= limit:
        return False
    planes = N * T * C
    return planes < limit and planes * (inner * es // 2) + 16 < limit


def flat_limit_ok(N, C, H, W, es):
    """flat_common_ok (csrc/shiftnd_flat.hip): the whole tensor below 2^32 bytes, planes below 2^26 bytes, dims below 2^15"""
    if N * C * H * W * es >= (1 << 32):
        return False
    return N * C < (1 << 31) and H < (1 << 15) and W < (1 << 15) and H * W * es < (1 << 26)


def frames_limit_ok(N, T, C, M, es):
    """frames_geometry_ok (csrc/shiftnd_frames.hip): 32-bit frame and workgroup indices, the tensor below 2^46 bytes"""
    limit = 1 << 31
    if T >= (1 << 30) or M >= limit or N >= limit or C >= limit or N * T >= limit:
        return False
    if N * T * ((M + 7) // 8) >= limit:
        return False
    return M <= (1 << 46) // (C * es) and N * T <= (1 << 46) // (M * C * es)


# ---------------------------------------------------------------------------------------------------------------------
# the cases.  shape: the PROBLEM [N, C, spatial ...] -- temporal families: [clips, C, T, pixels] -- whatever the memory order;
# layout: nchw (contiguous), nhwc (channels-last), segment (memory order N, T, C, M), frames (memory order N, T, M, C).
# marks: what the tensor is past; passes: (pass, paddings, active, the kernel shiftnd_last_kernel() must name -- one name, or one per
# padding where the host's rule reads the padding).  A pass allocates and draws its tensors once and runs once per padding.
# The kernel names are the ones DESIGN and the host's eligibility rules give (the comment at each row cites the rule).
# ---------------------------------------------------------------------------------------------------------------------
CASES = []
ALL = (0, 1, 2, 3, 4)


def _per_pad(zeros, other):
    return (zeros, other, other, other, other)


def _case(id, row, family, dt, layout, shape, marks, passes, wdt=None, knobs=(), cut=None, note=""):
    CASES.append(dict(id=id, row=row, family=family, dt=dt, layout=layout, shape=tuple(shape), marks=tuple(marks), passes=tuple(passes),
                      wdt=wdt or dt, knobs=tuple(knobs), cut=cut, note=note))


T8, M28 = 8, 28 * 28
# 1. fixed temporal shift, channels-last (csrc/shiftnd_frames.hip): frames_forward for pixel rows of whole 16-byte pieces,
#    frames_forward_ragged otherwise (C = 66: 132-byte rows, 4-byte pieces); grad_x is the call on the gradient under the negated table
_case("r1-f16-c64", 1, "temporal_fixed", "f16", "frames", (5351, 64, T8, M28), (EL31, BYTE32),
      [("forward", ALL, 0, "frames_forward"), ("gradx_negated", ALL, 0, "frames_forward")])
_case("r1-f16-c66", 1, "temporal_fixed", "f16", "frames", (5189, 66, T8, M28), (EL31, BYTE32),
      [("forward", ALL, 0, "frames_forward_ragged"), ("gradx_negated", ALL, 0, "frames_forward_ragged")])
_case("r1-u8", 1, "temporal_fixed", "u8", "frames", (10701, 64, T8, M28), (EL31, EL32, BYTE32), [("forward", ALL, 0, "frames_forward")])
# 2. learnable temporal shift, channels-last (SHIFTND_SHIFT_DIM0 | SHIFTND_FRAMES, csrc/shiftnd_frames_learn.hip)
_case("r2-bf16", 2, "temporal_learn", "bf16", "frames", (5351, 64, T8, M28), (EL31, BYTE32),
      [("forward", ALL, 1, "frames_active_forward"), ("backward", ALL, 1, "frames_backward"), ("backward", ALL, 0, "frames_backward")])
_case("r2-f32", 2, "temporal_learn", "f32", "frames", (2676, 64, T8, M28), (EL30, BYTE32),
      [("forward", ALL, 1, "frames_active_forward"), ("backward", ALL, 1, "frames_backward"), ("backward", ALL, 0, "frames_backward")])
# 3. learnable temporal shift, segment-major (SHIFTND_SHIFT_DIM0, csrc/shiftnd_tshift.hip): the last shape tshift_geometry_ok
#    accepts, 2^31 - 2^21 two-byte units
_case("r3-f16-last", 3, "temporal_learn", "f16", "segment", (1023, 64, T8, 64 * 64), (), wdt="f32",
      passes=[("forward", ALL, 1, "tshift_forward"), ("forward", ALL, 0, "tshift_forward"), ("backward", ALL, 1, "tshift_backward"),
              ("backward", ALL, 0, "tshift_backward")])
_case("r3-f32-last", 3, "temporal_learn", "f32", "segment", (1023, 64, T8, 32 * 64), (),
      passes=[("forward", ALL, 1, "tshift_forward"), ("forward", ALL, 0, "tshift_forward"), ("backward", ALL, 1, "tshift_backward"),
              ("backward", ALL, 0, "tshift_backward")])
# 4. fixed temporal shift, segment-major, unflagged (forward_common's last two routes): segment_forward up to the limit of
#    segment_forward_eligible, the 64-bit strided_gather_forward from it on
_case("r4-f16-last", 4, "temporal_fixed", "f16", "segment", (1023, 64, T8, 64 * 64), (), [("forward", ALL, 0, "segment_forward")])
_case("r4-f16-first", 4, "temporal_fixed", "f16", "segment", (1024, 64, T8, 64 * 64), (), [("forward", ALL, 0, "strided_gather_forward")])
_case("r4-u8-last", 4, "temporal_fixed", "u8", "segment", (1023, 64, T8, 64 * 64), (), [("forward", ALL, 0, "segment_forward")])
_case("r4-u8-first", 4, "temporal_fixed", "u8", "segment", (1024, 64, T8, 64 * 64), (), [("forward", ALL, 0, "strided_gather_forward")])
# 5. the 2-D shift on the headline route, config 2's kernels (csrc/shiftnd_step.hip, shiftnd_step_fwd.hip): step_forward_eligible
#    takes fp32 planes from 32 KiB -- 96 x 96 is the smallest square plane of whole pieces above that -- and step_forward_lds_eligible
#    the interpolating shift and 16-bit planes from 4 KiB; step_backward_eligible takes every 2-D plane of whole pieces
_case("r5-f32-4g", 5, "spatial", "f32", "nchw", (457, 256, 96, 96), (EL30, BYTE32),
      [("forward", ALL, 0, "step_gather_forward"), ("forward", ALL, 1, "step_active_forward"), ("backward", ALL, 0, "step_backward"),
       ("backward", ALL, 1, "step_backward")])
_case("r5-f32-8g", 5, "spatial", "f32", "nchw", (912, 256, 96, 96), (EL31, BYTE32),
      [("forward", ALL, 0, "step_gather_forward"), ("forward", ALL, 1, "step_active_forward"), ("backward", ALL, 0, "step_backward"),
       ("backward", ALL, 1, "step_backward")])
_case("r5-bf16", 5, "spatial", "bf16", "nchw", (2676, 256, 56, 56), (EL31, BYTE32),
      [("forward", ALL, 0, "step_gather_forward_lds"), ("forward", ALL, 1, "step_active_forward"), ("backward", ALL, 0, "step_backward"),
       ("backward", ALL, 1, "step_backward")])
# 6. the 3-D shift, config 3's geometry with N raised (csrc/shiftnd_walk.hip: walk16_geometry_ok; the sparse forward of 2-byte volumes
#    is step_forward_lds_eligible's)
_case("r6-bf16-3d", 6, "spatial", "bf16", "nchw", (84, 128, 16, 112, 112), (EL31, BYTE32),
      [("forward", ALL, 1, "walk_forward16"), ("forward", ALL, 0, "step_gather_forward_lds"), ("backward", (0, 2, 3), 1, "walk_backward16"),
       ("backward", (0, 2, 3), 0, "walk_backward16_sparse")])   # (the backward's 16 corner gathers a chunk: three paddings keep a pass at 5 s)
# 7. quantized 2-D (the names of tests/test_fullsize_properties.py::test_one_byte_rows_full_size: step_forward_eligible takes 1-byte
#    planes from 32 KiB under zeros padding, rows_forward_eligible the other paddings) and the fused quantized pool
#    (csrc/shiftnd_qpool.hip: planes above 48 KiB go to the band kernels, qpool_band_fast under zeros padding)
_case("r7-u8", 7, "quantized", "u8", "nchw", (168, 512, 224, 224), (EL31, EL32, BYTE32),
      [("forward", ALL, 0, _per_pad("step_gather_forward_small", "rows_gather_forward")),
       ("pool_forward", ALL, 0, _per_pad("qpool_band_fast", "qpool_band_forward"))])
# 8. the flat-stream kernels, both sides of 2^32 bytes (csrc/shiftnd_flat.hip: flat_common_ok): fp16 planes of 62 x 30 (60-byte rows);
#    ragged 16-bit rows are theirs by default.  Past the limit the per-channel kernels serve the shape: the sparse forward is
#    plane_forward_eligible's (a gather needs no whole source rows), the rest the small-plane band kernels' (csrc/shiftnd_small.hip)
_case("r8-f16-last", 8, "spatial", "f16", "nchw", (18040, 64, 62, 30), (), wdt="f32",
      passes=[("forward", ALL, 0, "flat_gather_forward"), ("forward", ALL, 1, "flat_active_forward"), ("backward", ALL, 1, "flat_backward"),
              ("backward", ALL, 0, "flat_backward")])
_case("r8-f16-first", 8, "spatial", "f16", "nchw", (18041, 64, 62, 30), (EL31, BYTE32), wdt="f32",
      passes=[("forward", ALL, 0, "plane_gather_forward"), ("forward", ALL, 1, "band_plane_forward"), ("backward", ALL, 1, "band_plane_backward"),
              ("backward", ALL, 0, "band_plane_backward")])
# 9. channels-last 2-D (csrc/shiftnd_cl_tiled.hip): each image is 401 408 bytes, far below the 2^31 bytes of one buffer resource
_case("r9-f16-cl", 9, "spatial", "f16", "nhwc", (10701, 64, 56, 56), (EL31, BYTE32), wdt="f32",
      passes=[("forward", ALL, 0, "cl_tiled_forward"), ("forward", ALL, 1, "cl_tiled_active_forward"), ("backward", ALL, 1, "cl_tiled_backward"),
              ("backward", ALL, 0, "cl_tiled_backward")])
# 10. fixed (grouped) shifts -- the input gradient without the input, a window cut 1 / 1 (csrc/shiftnd_gradx.hip) -- and the fused fp16
#     pool (tests/pooled16_cases.py: forward_route / backward_route)
_case("r10-f16-fixed", 10, "spatial", "f16", "nchw", (2676, 256, 56, 56), (EL31, BYTE32), cut=[[1, 1], [1, 1]],
      passes=[("backward_input", ALL, 0, "gradx_embed")])
_case("r10-f16-pool", 10, "spatial", "f16", "nchw", (2676, 256, 56, 56), (EL31, BYTE32), wdt="f32",
      passes=[("pool_forward", ALL, 0, "step_gather_forward_pool"), ("pool_forward", ALL, 1, "plane_pool_forward"),
              ("pool_backward", ALL, 0, "step_backward_pool"), ("pool_backward", ALL, 1, "crop_backward_pool"),
              ("pool_backward_input", ALL, 0, "gradx_embed_pool")])

BY_ID = {c["id"]: c for c in CASES}
PASSES = [(c["id"], i) for c in CASES for i in range(len(c["passes"]))]

# the boundary shapes of rows 3, 4 and 8: (limit function, arguments of the last accepted shape, of the first refused one)
BOUNDARIES = {
    "tshift fp16": (tshift_limit_ok, (1023, T8, 64, 64 * 64, 2), (1024, T8, 64, 64 * 64, 2)),
    "tshift fp32": (tshift_limit_ok, (1023, T8, 64, 32 * 64, 4), (1024, T8, 64, 32 * 64, 4)),
    "segment fp16": (segment_limit_ok, (1023, T8, 64, 64 * 64, 2), (1024, T8, 64, 64 * 64, 2)),
    "segment uint8": (segment_limit_ok, (1023, T8, 64, 64 * 64, 1), (1024, T8, 64, 64 * 64, 1)),
    "flat fp16": (flat_limit_ok, (18040, 64, 62, 30, 2), (18041, 64, 62, 30, 2)),
}
DECLINED_TSHIFT = {"f16": (1024, 64, T8, 64 * 64), "f32": (1024, 64, T8, 32 * 64)}   # the first shapes SHIFTND_SHIFT_DIM0 refuses


def numel(case):
    return int(np.prod(case["shape"], dtype=np.int64))


def nbytes(case):
    return numel(case) * es_of(DTYPES[case["dt"]])


def sample_numel(case):
    return numel(case) // case["shape"][0]


def chunk_samples(case, chunk_bytes=CHUNK_BYTES):
    """samples (clips) per chunk: as many as fit `chunk_bytes` of the tensor's type, at least one"""
    return max(1, chunk_bytes // (sample_numel(case) * es_of(DTYPES[case["dt"]])))


def chunks(case, chunk_bytes=CHUNK_BYTES):
    n, k = case["shape"][0], chunk_samples(case, chunk_bytes)
    return [(i, a, min(a + k, n)) for i, a in enumerate(range(0, n, k))]


def marked_samples(case):
    """the samples the C oracle checks: the first, the last, and those that hold element 2^31, element 2^32 and byte 2^32"""
    n, per, es = case["shape"][0], sample_numel(case), es_of(DTYPES[case["dt"]])
    picks = {0, n - 1}
    for at in ((1 << 31), (1 << 32), (1 << 32) // es):
        if at // per < n:
            picks.add(at // per)
    return sorted(picks)


def weights_of(case):
    """the table of a case, on the CPU: float weights ([C, nd], temporal: [C]) or int64 shifts (fixed temporal, quantized)"""
    C, sp = case["shape"][1], case["shape"][2:]
    seed = 7 + case["row"]
    if case["family"] == "temporal_learn":
        return temporal_weights(C, sp[0], seed)
    if case["family"] == "temporal_fixed":
        return temporal_shifts(C, sp[0], seed)
    if case["family"] == "quantized":
        return spatial_shifts(C, sp, seed)
    w = spatial_weights(C, sp, seed)
    if any(p[0] in ("backward_input", "pool_backward_input") for p in case["passes"]):
        w = torch.round(w)          # the fixed ops' integer table, as floats
    return w
