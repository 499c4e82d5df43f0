"""Self-checks of tests/bigindex_cases.py that need no GPU: the torch reference against the C oracle and against the slicing idiom of
tests/test_tshift_gpu.py on shapes of a few hundred elements (every padding, both shifts, cut windows, the quantized gather, the
temporal forms, the fused pools), the reference of a slice against the slice of the reference, every boundary shape against its
limit formula, and every big case against the marks its row names."""
import itertools

import numpy as np
import pytest
import torch

import bigindex_cases as B
import pooled16_cases as PC
from oracle import oracle as O

SWEEP = [(pad, active) for pad in range(5) for active in (0, 1)]
# nd, shape, cut
SMALL = [(1, (2, 3, 9), None), (1, (2, 3, 9), [[2, 1]]), (2, (2, 4, 6, 7), None), (2, (2, 4, 6, 7), [[1, 1], [0, 2]]),
         (2, (1, 3, 1, 8), None), (3, (1, 3, 3, 4, 5), None), (3, (2, 3, 3, 4, 5), [[1, 0], [0, 1], [1, 1]])]


def _small_inputs(nd, shape, cut, seed):
    b, new = O.check_borders(list(shape), cut, nd)
    x = B.eighths(seed, 0, shape, B.F64, "cpu")
    go = B.eighths(seed, 1, new, B.F64, "cpu")
    w = B.spatial_weights(shape[1], shape[2:], seed).to(B.F64)
    return b, x, go, w


@pytest.mark.parametrize("nd,shape,cut", SMALL, ids=lambda v: str(v).replace(" ", ""))
def test_the_reference_is_the_oracle(nd, shape, cut):
    b, x, go, w = _small_inputs(nd, shape, cut, 11 + nd)
    xn, gn, wn = x.numpy(), go.numpy(), w.numpy()
    for pad, active in SWEEP:
        what = (nd, shape, cut, pad, active)
        out = B.shift_forward(x, w, pad, active, nd, b)
        assert np.array_equal(out.numpy(), O.forward(xn, wn, pad, active, b)), what
        gx, gw = B.shift_backward(go, x, w, pad, active, nd, b)
        gx_o, gw_o = O.backward(gn, wn, xn, pad, active, b)
        assert np.array_equal(gx.numpy(), gx_o), what
        assert np.array_equal(gw.numpy(), gw_o), what      # (exact data: every partial sum is exact, whatever the order)
        alone, none = B.shift_backward(go, None, w, pad, active, nd, b, sizes=shape[2:])   # the input gradient without the input
        assert none is None and torch.equal(alone, gx), what
        # ... and narrowed: the fp32 oracle's bits, representable in both 16-bit types
        o32 = O.forward(xn.astype(np.float32), wn.astype(np.float32), pad, active, b)
        assert np.array_equal(B.narrow(out, B.F32).numpy(), o32), what
        for dt in (B.F16, B.BF16):
            assert torch.equal(B.narrow(out, dt).to(B.F64), out) and torch.equal(B.narrow(gx, dt).to(B.F64), gx), what + (dt,)


@pytest.mark.parametrize("npdt", [np.uint8, np.int8])
def test_the_quantized_gather_is_the_oracle(npdt):
    tdt = torch.uint8 if npdt == np.uint8 else torch.int8
    for nd, shape, cut in SMALL:
        b, _ = O.check_borders(list(shape), cut, nd)
        xq = B.bytes_(5, nd, shape, tdt, "cpu")
        shifts = B.spatial_shifts(shape[1], shape[2:], 3)
        for pad in range(5):
            got = B.shift_forward(xq, shifts, pad, False, nd, b, fill=9)
            want = O.forward_q(xq.numpy(), (shifts + 128).numpy(), 128, 9, pad, b)
            assert got.dtype == tdt and np.array_equal(got.numpy(), want), (nd, shape, cut, pad)
    # the table holds what the issue asks for: 0, a shift beyond the dim, a negative one, neighbours that differ
    s = B.spatial_shifts(8, (56, 56), 3)
    assert (s[0] == 0).all() and (s[1] > 56).all() and (s[2] < 0).all() and not torch.equal(s[4], s[5])


def test_the_temporal_forms_are_the_slicing_idiom_and_the_oracle():
    from test_tshift_gpu import _reference
    shape = (2, 3, 5, 4)                        # (N, T, C, M) in memory
    N, T, C, M = shape
    x = B.eighths(21, 0, shape, B.F64, "cpu")
    go = B.eighths(21, 1, shape, B.F64, "cpu")
    w = B.temporal_weights(C, T, 4)
    assert w[0] == 0 and w[2] == T + 1 and w[3] == -(T + 1) and w[4] == 0.5
    for pad, active in SWEEP:
        want_out, want_gx, gw64 = _reference(x.numpy(), go.numpy(), w.numpy(), pad, active, B.F32)
        xv, gv = x.transpose(1, 2), go.transpose(1, 2)            # the problem [N, C, T, M]
        out = B.temporal_forward(xv, w, pad, active)
        gx, gw = B.temporal_backward(gv, xv, w, pad, active)
        assert np.array_equal(out.transpose(1, 2).numpy(), want_out.astype(np.float64)), (pad, active)
        assert np.array_equal(gx.transpose(1, 2).numpy(), want_gx.astype(np.float64)), (pad, active)
        assert np.array_equal(gw.numpy(), gw64), (pad, active)
        # the same values in channels-last memory: the reference reads views, the layout changes nothing
        xf = x.permute(0, 1, 3, 2).contiguous().permute(0, 3, 1, 2)    # memory (N, T, M, C), seen as [N, C, T, M]
        assert torch.equal(B.temporal_forward(xf, w, pad, active), out), (pad, active)
    # the fixed table: integer shifts, the quantized gather with its fill
    s = B.temporal_shifts(24, T, 5)
    assert s[0] == 0 and s[1] == T + 1 and s[2] == -(T + 1) and len(set(s[16:24].tolist())) == 1 and len(set(s[:16].tolist())) > 4
    xq = B.bytes_(6, 0, (2, 24, T, 5), torch.uint8, "cpu")
    for pad in range(5):
        w2 = np.stack([s.numpy() + 128, np.full(24, 128)], 1)
        assert np.array_equal(B.temporal_forward_q(xq, s, 7, pad).numpy(), O.forward_q(xq.numpy(), w2, 128, 7, pad)), pad
        xf = xq.to(B.F64)
        w2f = torch.stack([s.to(B.F64), torch.zeros(24, dtype=B.F64)], 1).numpy()
        assert np.array_equal(B.temporal_forward(xf, s.to(B.F64), pad, 0).numpy(), O.forward(xf.numpy(), w2f, pad, False)), pad


def test_the_fused_pools_are_the_two_step_sequence():
    from test_pooled_gpu import quantized_pool_references
    shape = (2, 3, 6, 8)
    x = B.eighths(31, 0, shape, B.F32, "cpu")
    gp = B.eighths(31, 1, (2, 3, 3, 4), B.F32, "cpu")
    w = B.spatial_weights(3, shape[2:], 9)
    b = O.default_borders(x.numpy())
    for dt, (pad, active) in itertools.product((B.F16, B.BF16, B.F32), SWEEP):
        y, ref, g, gx_ref, gw64 = PC.two_step_reference(x.numpy(), w.numpy(), gp.numpy(), pad, active, (2, 2), b, dt)
        assert np.array_equal(B.pooled_forward(x.to(dt), w, pad, active, dt).float().numpy(), ref), (dt, pad, active)
        gx, gw = B.pooled_backward(gp.to(dt), x.to(dt), w, pad, active, dt)
        assert np.array_equal(B.narrow(gx, dt).float().numpy(), gx_ref) and np.array_equal(gw.numpy(), gw64), (dt, pad, active)
    xq = B.bytes_(8, 0, shape, torch.uint8, "cpu")
    s = B.spatial_shifts(3, shape[2:], 3)
    for pad in range(5):
        refs = quantized_pool_references(xq.numpy(), (s + 128).numpy().astype(np.uint8), 7, pad, (2, 2), b, list(shape))
        for inside, ref in zip((True, False), refs):
            assert np.array_equal(B.pooled_forward_q(xq, s, 7, pad, inside).numpy(), ref), (pad, inside)


@pytest.mark.parametrize("nd,shape,cut", [(2, (5, 4, 6, 7), [[1, 1], [0, 2]]), (3, (4, 3, 3, 4, 5), None)], ids=["2d", "3d"])
def test_a_slice_of_samples_needs_nothing_from_outside(nd, shape, cut):
    b, x, go, w = _small_inputs(nd, shape, cut, 41)
    for pad, active in SWEEP:
        out = B.shift_forward(x, w, pad, active, nd, b)
        gx, gw = B.shift_backward(go, x, w, pad, active, nd, b)
        total = torch.zeros_like(gw)
        for a, e in ((0, 1), (1, 3), (3, shape[0])):
            assert torch.equal(B.shift_forward(x[a:e], w, pad, active, nd, b), out[a:e]), (pad, active, a)
            gxs, gws = B.shift_backward(go[a:e], x[a:e], w, pad, active, nd, b)
            assert torch.equal(gxs, gx[a:e]), (pad, active, a)
            total += gws
        assert torch.equal(total, gw), (pad, active)       # fp64 sums of exact terms: the chunks' sums add up to the whole
    xv = x.reshape(shape[0], shape[1], shape[2], -1)
    wt = B.temporal_weights(shape[1], shape[2], 2)
    whole = B.temporal_forward(xv, wt, 3, 1)
    assert torch.equal(B.temporal_forward(xv[2:4], wt, 3, 1), whole[2:4])


def test_the_data_is_the_exact_data_and_repeats():
    for dev_dt in (B.F16, B.BF16, B.F32):
        a = B.eighths(3, 5, (4, 6, 7), dev_dt, "cpu", 0, 7)
        assert torch.equal(a, B.eighths(3, 5, (4, 6, 7), dev_dt, "cpu", 0, 7)) and not torch.equal(a, B.eighths(3, 6, (4, 6, 7), dev_dt, "cpu", 0, 7))
        k = a.double() * 8
        assert torch.equal(k, torch.round(k)) and k.min() >= 0 and k.max() <= 7
    w = B.spatial_weights(16, (56, 56), 1)
    assert (w[0] == 0).all() and (w[1] > 57).all() and (w[2] == -28).all() and (w[3] * 2 % 2 == 1).all()
    assert torch.equal(w.to(B.BF16).float(), w) and not torch.equal(w[4], w[5])
    assert torch.equal(torch.round(w)[1], torch.round(w[1])) and (torch.round(w)[2] < 0).all()


@pytest.mark.parametrize("name", sorted(B.BOUNDARIES))
def test_boundary_shapes_lie_on_their_sides_of_the_limit(name):
    ok, last, first = B.BOUNDARIES[name]
    assert ok(*last), (name, "the last accepted shape is outside the limit", last)
    assert not ok(*first), (name, "the first refused shape is inside the limit", first)
    assert first[0] == last[0] + 1         # one clip (sample) apart: nothing lies between them


def test_boundary_shapes_are_the_table_s():
    for dt in ("f16", "f32"):
        N, C, T, M = B.BY_ID["r3-%s-last" % dt]["shape"]
        es = B.es_of(B.DTYPES[dt])
        assert B.tshift_limit_ok(N, T, C, M, es) and not B.tshift_limit_ok(*[(N + 1), T, C, M, es])
        assert B.DECLINED_TSHIFT[dt] == (N + 1, C, T, M)
        assert N * T * C * M * es // 2 == 2 ** 31 - 2 ** 21 and N * T * C * M * es == 2 ** 32 - 2 ** 22
        assert B.frames_limit_ok(N + 1, T, C, M, es)          # the channels-last route takes the refused tensor
    for dt in ("f16", "u8"):
        es = B.es_of(B.DTYPES[dt])
        for side, want in (("last", True), ("first", False)):
            N, C, T, M = B.BY_ID["r4-%s-%s" % (dt, side)]["shape"]
            assert B.segment_limit_ok(N, T, C, M, es) is want, (dt, side)
    N, C, T, M = B.BY_ID["r4-u8-last"]["shape"]
    assert N * T * C * M == 2 ** 31 - 2 ** 21
    for side, want, nb in (("last", True, 4294963200), ("first", False, 4295201280)):
        c = B.BY_ID["r8-f16-%s" % side]
        assert B.flat_limit_ok(*c["shape"], 2) is want and B.nbytes(c) == nb, side
    for c in B.CASES:
        if c["layout"] == "frames":
            N, C, T, M = c["shape"]
            assert B.frames_limit_ok(N, T, C, M, B.es_of(B.DTYPES[c["dt"]])), c["id"]


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c["id"])
def test_every_case_crosses_the_marks_it_names(case):
    n, nb, per = B.numel(case), B.nbytes(case), B.sample_numel(case)
    es = B.es_of(B.DTYPES[case["dt"]])
    N = case["shape"][0]
    plane = int(np.prod(case["shape"][2:]))
    for mark in case["marks"]:
        at = (1 << 32) // es if mark == B.BYTE32 else B.MARKS[mark]       # the first element past the mark
        assert (nb > (1 << 32)) if mark == B.BYTE32 else (n > at), (case["id"], mark, n, nb)
        # the mark lies inside a plane, not between two; "just over": the highest mark lies in one of the last two samples
        assert at % plane != 0 and at % per != 0, (case["id"], mark)
        if at == max((1 << 32) // es if m == B.BYTE32 else B.MARKS[m] for m in case["marks"]):
            assert at // per in (N - 1, N - 2), (case["id"], mark, at // per, N)
    for mark, at in B.MARKS.items():        # ... and names every element mark it is past (the boundary shapes: none)
        if n > at and mark != B.EL30:
            assert mark in case["marks"], (case["id"], mark)
    assert (nb > (1 << 32)) == (B.BYTE32 in case["marks"]), case["id"]
    # chunks: whole samples, at most 256 MiB each, all of the tensor once
    cover = B.chunks(case)
    assert cover[0][1] == 0 and cover[-1][2] == N and all(a[2] == b_[1] for a, b_ in zip(cover, cover[1:]))
    assert all((e - a) * per * es <= (256 << 20) for _, a, e in cover)
    picks = B.marked_samples(case)
    assert picks[0] == 0 and picks[-1] == N - 1 and all(0 <= p < N for p in picks)
    if B.BYTE32 in case["marks"]:
        assert ((1 << 32) // es) // per in picks


def test_the_table_holds_the_ten_rows():
    assert sorted({c["row"] for c in B.CASES}) == list(range(1, 11))
    assert len({c["id"] for c in B.CASES}) == len(B.CASES)
    one_byte = [c for c in B.CASES if c["dt"] == "u8" and c["marks"]]
    assert one_byte and all(B.EL32 in c["marks"] and B.BYTE32 in c["marks"] for c in one_byte)
    assert any(c["dt"] == "f32" and B.EL31 in c["marks"] for c in B.CASES)
    for c in B.CASES:
        w = B.weights_of(c)
        assert w.shape[0] == c["shape"][1], c["id"]
