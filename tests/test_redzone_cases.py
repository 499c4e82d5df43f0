"""Self-checks of tests/redzone.py on CPU tensors (no GPU): the geometry of Guarded, what the two patterns are in every dtype, that
assert_intact sees one changed byte at either edge of either red zone, and that run_guarded accepts a correct "kernel" written with
the oracle and rejects each way a kernel can leave its tensors -- by the check named for it, and by the right pattern."""
import numpy as np
import pytest
import torch

import redzone as RZ
from oracle import oracle as O

CPU = "cpu"
DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int8, torch.uint8, torch.int32]
SHAPES = {1: (2, 3, 45), 2: (2, 3, 7, 11), 3: (2, 3, 4, 5, 6)}


# (torch has no channels-last layout of [N, C, L])
@pytest.mark.parametrize("layout,nd", [("contiguous", 1), ("contiguous", 2), ("contiguous", 3), ("channels_last", 2), ("channels_last", 3)])
def test_geometry(layout, nd):
    shape = SHAPES[nd]
    fmt = {"contiguous": torch.contiguous_format, "channels_last": torch.channels_last if nd == 2 else torch.channels_last_3d}[layout]
    for dtype in DTYPES:
        es = torch.empty(0, dtype=dtype).element_size()
        for offset in (0, 16, es):
            g = RZ.Guarded(shape, dtype, CPU, layout, offset)
            fresh = torch.empty(shape, dtype=dtype, memory_format=fmt)
            assert g.t.shape == fresh.shape and g.t.stride() == fresh.stride() and g.t.dtype == dtype
            assert g.t.is_contiguous(memory_format=fmt)
            assert g.t.data_ptr() % 512 == offset
            assert g.nbytes == fresh.numel() * es
            assert g.red == RZ.round_up(4096 + int(np.prod(shape[2:])) * es, 512) and g.red % 512 == 0
            assert g.buf.numel() == 2 * g.red + g.nbytes and g.buf.data_ptr() + g.red == g.t.data_ptr()
            # dense: writing every element of .t writes every byte of the interior and nothing else
            g.paint(0x7B).poison()
            g.t.zero_()
            assert bool((g.interior_bytes() == 0).all())
            g.assert_intact(("geometry",))


def test_tables_and_workspaces_take_one_pass():
    for shape, dtype in (((4, 2), torch.float16), ((4, 3), torch.float64), ((1000,), torch.uint8), ((0,), torch.uint8)):
        g = RZ.Guarded(shape, dtype, CPU)
        assert g.red == 4096 and g.t.data_ptr() % 512 == 0
        g.paint(0xFF).poison().assert_intact(("table",))


def test_patterns():
    assert RZ.PATTERNS == (0xFF, 0x7B)
    finite = {torch.float16: 61280.0, torch.bfloat16: 1.3e36, torch.float32: 1.3e36, torch.float64: 6.5e286}
    for dtype, about in finite.items():
        nan = torch.full((64,), 0xFF, dtype=torch.uint8).view(dtype)
        assert bool(torch.isnan(nan).all()), dtype
        assert bool(torch.isnan(nan * 0).all())                            # 0 * garbage
        big = torch.full((64,), 0x7B, dtype=torch.uint8).view(dtype).double()
        assert bool(torch.isfinite(big).all()) and bool(((big - about).abs() <= 0.05 * about).all()), (dtype, big[0])
        if dtype == torch.float16:
            assert float(big[0]) == 61280.0
    for dtype in (torch.int8, torch.uint8):
        assert int(torch.full((1,), 0x7B, dtype=torch.uint8).view(dtype)[0]) == 123
    assert all(p != 0 for p in RZ.PATTERNS)


def test_assert_intact_sees_one_byte():
    g = RZ.Guarded((2, 3, 7, 11), torch.float16, CPU).paint(0x7B).poison()
    g.assert_intact(("untouched",))
    places = {"the byte before the interior": (g.red - 1, -1), "the byte after it": (g.red + g.nbytes, g.nbytes),
              "the far end of the left red zone": (0, -g.red), "the far end of the right red zone": (g.buf.numel() - 1, g.nbytes + g.red - 1)}
    for place, (at, offset) in places.items():
        g.buf[at] = 0
        with pytest.raises(AssertionError, match=r"first at offset %d, last at offset %d .*fake_kernel" % (offset, offset)):
            g.assert_intact(("grad_x", "fake_kernel", place))
        assert bool(g.dirty())
        g.buf[at] = 0x7B
        g.assert_intact(("restored",))
        assert not bool(g.dirty())
    g.t.fill_(1.0)   # the interior is the kernel's
    g.assert_intact(("interior written",))


# ---------------------------------------------------------------------------------------------------------------------
# run_guarded on fake kernels: the oracle's 2-D forward on guarded CPU tensors, and five ways to be wrong
# ---------------------------------------------------------------------------------------------------------------------
SHAPE, PAD, ACTIVE = (2, 3, 7, 11), 0, 1


def _beyond(g, k=0):
    """the element k places after the end of a guarded tensor, as a kernel with a raw pointer reaches it"""
    return g.t.as_strided((1,), (1,), g.t.storage_offset() + g.t.numel() + k)


def _fixture():
    rs = np.random.RandomState(3)
    x = (rs.randint(-7, 8, size=SHAPE) / 8.0).astype(np.float32)
    w = (rs.randint(-10, 11, size=(SHAPE[1], 2)) / 4.0).astype(np.float32)
    gx, go = RZ.Guarded(SHAPE, torch.float32, CPU), RZ.Guarded(SHAPE, torch.float32, CPU)
    gw = RZ.Guarded(w.shape, torch.float32, CPU)
    return x, w, gx, gw, go, torch.from_numpy(O.forward(x, w, PAD, ACTIVE))


def _run(mutation, patterns=RZ.PATTERNS):
    x, w, gx, gw, go, ref = _fixture()

    def kernel():
        out = torch.from_numpy(O.forward(gx.t.numpy().copy(), gw.t.numpy().copy(), PAD, ACTIVE))
        if mutation == "leaves an element unwritten":
            keep = go.t[1, 2, 6, 10].clone()
        if mutation == "adds 0 * the element after the input":
            out = out + 0 * _beyond(gx)
        if mutation == "takes max with the element after the input":
            out = torch.fmax(out, _beyond(gx))   # (fmax: the GPU's max returns the other operand of a NaN)
        go.t.copy_(out)
        if mutation == "leaves an element unwritten":
            go.t[1, 2, 6, 10] = keep
        if mutation == "writes one element past out":
            _beyond(go)[0] = out.reshape(-1)[-1]
        if mutation == "writes one element before out":
            _beyond(go, -go.t.numel() - 1)[0] = 0.0
        if mutation == "writes its input":
            gx.t[0, 0, 0, 0] += 1.0
        if mutation == "writes the table's red zone":
            _beyond(gw, 1)[0] = 0.0
        return "fake_forward"

    return RZ.run_guarded(kernel, [("x", gx, torch.from_numpy(x)), ("w", gw, torch.from_numpy(w))], [("out", go)], [ref],
                          (SHAPE, PAD, ACTIVE, mutation), patterns=patterns)


def test_run_guarded_accepts_the_oracle():
    assert _run(None) == "fake_forward"
    for byte in RZ.PATTERNS:
        assert _run(None, patterns=(byte,)) == "fake_forward"


@pytest.mark.parametrize("mutation,message", [
    ("writes one element past out", r"red zone of 'out' written: 4 bytes, first at offset %d" % (int(np.prod(SHAPE)) * 4)),
    ("writes one element before out", r"red zone of 'out' written: .*first at offset -4, last at offset -"),
    ("writes the table's red zone", r"red zone of 'w' written"),
    ("writes its input", r"input written.*'x'"),
    ("leaves an element unwritten", r"'out'.*1 of 462 differ, first at \(1, 2, 6, 10\): nan"),
])
def test_run_guarded_rejects_under_either_pattern(mutation, message):
    for patterns in (RZ.PATTERNS, RZ.PATTERNS[:1], RZ.PATTERNS[1:]):
        with pytest.raises(AssertionError, match=message):
            _run(mutation, patterns)


def test_a_leak_through_arithmetic_needs_the_nan_pattern():
    mutation = "adds 0 * the element after the input"
    assert _run(mutation, patterns=(0x7B,)) == "fake_forward"      # 0 * 1.3e36 == 0: the finite pattern cannot see it
    with pytest.raises(AssertionError, match=r"'out'.*462 of 462 differ.*pattern 0xFF"):
        _run(mutation, patterns=(0xFF,))
    with pytest.raises(AssertionError, match=r"pattern 0xFF"):
        _run(mutation)


def test_a_leak_through_max_needs_the_finite_pattern():
    mutation = "takes max with the element after the input"
    assert _run(mutation, patterns=(0xFF,)) == "fake_forward"      # max(v, NaN) == v: the NaN pattern cannot see it
    with pytest.raises(AssertionError, match=r"'out'.*462 of 462 differ.*pattern 0x7B"):
        _run(mutation, patterns=(0x7B,))
    with pytest.raises(AssertionError, match=r"pattern 0x7B"):
        _run(mutation)


def test_a_refused_call_must_launch_nothing():
    x, w, gx, gw, go, ref = _fixture()

    def refuses():
        raise RuntimeError("shiftnd_backward_pooled failed: not served (-5)")

    def refuses_late():
        go.t[0, 0, 0, 0] = 1.0
        refuses()

    ins = [("x", gx, torch.from_numpy(x)), ("w", gw, torch.from_numpy(w))]
    assert RZ.run_guarded(refuses, ins, [("out", go)], [ref], ("refused",), raises="not served") is None
    with pytest.raises(AssertionError, match="written by a refused call"):
        RZ.run_guarded(refuses_late, ins, [("out", go)], [ref], ("refused",), raises="not served")
    with pytest.raises(AssertionError, match="did not raise"):
        RZ.run_guarded(lambda: "k", ins, [("out", go)], [ref], ("refused",), raises="not served")
