"""The host side of the flagged C ABI (SHIFTND_SHIFT_DIM0 and the bits beside it), pinned against recorded answers: the status of
shiftnd_forward, shiftnd_forward_quantized and shiftnd_backward and the bytes of shiftnd_backward_workspace_bytes for an enumerated
list of problems.  Every tensor and table pointer is NULL, so nothing can be launched: an accepted geometry ends in INVALID_ARGUMENT
or, when empty, in OK before any device call.  No GPU is needed.

tests/golden/temporal_abi_status.json holds one row per case, in the order of cases(): [workspace bytes, then forward, quantized
forward and backward under segment-major strides, then the same three under channels-last strides].  It was recorded from the build
before csrc/shiftnd_api.hip's flagged calls were merged (tests/golden/make_golden_temporal_abi.py); the file and the list must agree
in length and order.

The list.  Flag sets: every subset of SHIFT_DIM0, FRAMES, PER_CLIP, WEIGHTS_F32 that holds SHIFT_DIM0, and PER_CLIP alone (9).
Element types: the four float and three integer ones.  The plain problem N, C, T, M = 2, 3, 4, 5 runs under the whole product with
ndim 1, 2, 3, active 0 / 1 and padding mode 0 / 4.  The other sizes run with ndim 2 and 3 (ndim 1 has no M, and the flag refuses it
before it looks at a size; the sizes with a 0 in N, C or T run with ndim 1 too) and with the two pairs (active, padding) = (0, 0) and
(1, 4): neither enters a size check, and the pairs keep the file at a few thousand rows.
"""
import ctypes
import hashlib
import itertools
import json
import os

from torchshifts import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_abi_status.json")

BITS = (abi.FRAMES, abi.PER_CLIP, abi.WEIGHTS_F32)
FLAG_SETS = [abi.SHIFT_DIM0 | sum(s) for r in range(4) for s in itertools.combinations(BITS, r)] + [abi.PER_CLIP]
DTYPES = (abi.F32, abi.F64, abi.F16, abi.BF16, abi.I8, abi.U8, abi.I32)
PLAIN = (2, 3, 4, 5)
WHOLE = None   # the window is the whole input

# (N, C, T, M, window of T or None)
SIZES = (
    [tuple(0 if i == k else v for i, v in enumerate(PLAIN)) + (WHOLE,) for k in range(4)] +    # each of N, C, T, M equal to 0
    [tuple(1 if i == k else v for i, v in enumerate(PLAIN)) + (WHOLE,) for k in range(4)] +    # ... equal to 1
    [(2, 3, 17, 5, WHOLE),                       # more frames than the in-place kernel's register slots
     (2, 3, 4, 5, (1, 3)),                       # a cropped window
     (1 << 16, 1, 1 << 15, 1, WHOLE),            # N * T = 2^31
     (1, 1, 16, (1 << 27) - 2, WHOLE),           # 2^31 - 32 two-byte units: the last tensor the 32-bit unit count serves
     (1, 1, 16, (1 << 27) - 1, WHOLE),           # 2^31 - 16 two-byte units
     (1, 1, 16, 1 << 27, WHOLE),                 # ... and the next size up
     (1 << 16, 1 << 15, 1, 1, WHOLE)])           # N * C = 2^31 (what SHIFTND_PER_CLIP's table index rests on)


def cases():
    """(flags | dtype, ndim, active, padding mode, (N, C, T, M, window)) in the order of the recorded file"""
    out = []
    for flags, dt, nd, active, pad in itertools.product(FLAG_SETS, DTYPES, (1, 2, 3), (0, 1), (0, 4)):
        out.append((flags | dt, nd, active, pad, PLAIN + (WHOLE,)))
    for size in SIZES:
        dims = (1, 2, 3) if 0 in size[:3] else (2, 3)
        for flags, dt, nd, (active, pad) in itertools.product(FLAG_SETS, DTYPES, dims, ((0, 0), (1, 4))):
            out.append((flags | dt, nd, active, pad, size))
    return out


def problem_and_strides(dtype, nd, active, pad, size):
    """the shiftnd_problem of a case, its segment-major strides (memory order N, T, C, M) and its channels-last ones (N, T, M, C)"""
    n, c, t, m, window = size
    inner = () if nd == 1 else ((m,) if nd == 2 else ((2, m // 2) if m % 2 == 0 and m > 0 else (1, m)))
    if nd == 1:
        m = 1
    p = abi.Problem()
    p.ndim, p.dtype, p.padding_mode, p.active = nd, dtype, pad, active
    for i, v in enumerate((n, c, t) + inner):
        p.sizes[i] = v
    for i in range(3):
        p.borders[2 * i], p.borders[2 * i + 1] = 0, 1
    for i, v in enumerate((t,) + inner):
        p.borders[2 * i], p.borders[2 * i + 1] = 0, v
    if window:
        p.borders[0], p.borders[1] = window
    last = inner[-1] if nd == 3 else 1
    segment = [t * c * m, m, c * m] + ([] if nd == 1 else ([1] if nd == 2 else [last, 1]))
    frames = [t * m * c, 1, m * c] + ([] if nd == 1 else ([c] if nd == 2 else [last * c, c]))
    as_array = lambda st: (ctypes.c_int64 * 5)(*(st + [0] * (5 - len(st))))   # noqa: E731
    return p, as_array(segment), as_array(frames)


def answers(case):
    """what the library says to one case: [workspace bytes, forward, quantized forward, backward (segment-major), the three again
    (channels-last)]; every pointer but the problem and the stride arrays is NULL"""
    L = abi.lib()
    p, segment, frames = problem_and_strides(*case)
    row = [int(L.shiftnd_backward_workspace_bytes(ctypes.byref(p)))]
    for st in (segment, frames):
        row.append(int(L.shiftnd_forward(ctypes.byref(p), None, st, None, None, st, None)))
        row.append(int(L.shiftnd_forward_quantized(ctypes.byref(p), None, st, None, abi.U8, 0, 0, None, st, None)))
        row.append(int(L.shiftnd_backward(ctypes.byref(p), None, st, None, st, None, None, st, None, None, 0, None)))
    return row


def digest(listed):
    return hashlib.sha256(json.dumps(listed).encode()).hexdigest()


def test_the_case_list_is_the_enumerated_one():
    listed = cases()
    assert len(FLAG_SETS) == 9 and len(set(FLAG_SETS)) == 9 and all(f & abi.SHIFT_DIM0 for f in FLAG_SETS[:-1])
    assert len(listed) == len(set(listed)) and 2000 < len(listed) < 6000


def test_every_status_and_every_byte_count_is_the_recorded_one():
    with open(GOLDEN) as f:
        recorded = json.load(f)
    listed = cases()
    assert len(recorded["rows"]) == len(listed), "the case list and the recorded file disagree in length"
    assert recorded["cases_sha256"] == digest(listed), "the case list and the recorded file disagree in order"
    now = [answers(c) for c in listed]
    wrong = [(c, row, got) for c, row, got in zip(listed, recorded["rows"], now) if got != row]
    assert not wrong, "%d of %d cases differ; the first: case %r recorded %r now %r" % ((len(wrong), len(listed)) + wrong[0])
    # the list reaches every kind of answer: accepted (NULL tensors refused), empty, unsupported, and a plan of some size
    seen = {v for row in recorded["rows"] for v in row[1:]}
    assert seen == {0, -1, -2}
    assert any(row[0] > 8 for row in recorded["rows"]) and any(row[0] == 8 for row in recorded["rows"])
