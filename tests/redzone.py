"""Red zones: tensors laid inside one allocation of the test's own, between two painted margins, so that a kernel's store past either
end -- or a load past either end that reaches a result -- becomes a failed assertion (tests/test_redzone_gpu.py on the GPU;
tests/test_redzone_cases.py checks this module itself on CPU tensors).  No GPU dependency: every function works on any device.

  Guarded ........ one flat uint8 buffer: red zone | interior | red zone; `.t` is a dense view of the interior
  PATTERNS ....... the two bytes the red zones (and with them every byte a stray load can reach) are painted with
  run_guarded .... one call under both patterns: red zones intact, inputs unchanged, outputs equal to the expectation, and the two
                   runs' outputs byte-identical

0xFF repeated is NaN in every float type: a stray value that meets arithmetic (0 * garbage, a window sum) turns the result into NaN.
min / max / compare / select swallow NaN, and the integer kernels have none: 0x7B repeated is a huge finite value (61280 in fp16,
about 1.3e36 in bf16 / fp32, 6.5e286 in fp64) and 123 as a byte.  Neither is zero, so stray stores of zeros or of a fill value show.

A red zone is 4096 bytes (one pass of a 256-thread workgroup at 16 bytes per thread) plus one (n, c) plane of the tensor (the next
unit a wrong index can be off by), rounded up to 512; weight tables, grad_w and workspaces (fewer than three dims) take 4096.
What cannot be seen: a load beyond a tensor that is masked out before it reaches a result, and anything beyond the red zones."""
import numpy as np
import torch

PATTERNS = (0xFF, 0x7B)
POISON = 0xFF   # outputs before the call: an element no kernel wrote is NaN (floats) or -1 / 255
ALIGN = 512     # what a fresh allocation of torch's caching allocator is aligned to
PASS_BYTES = 4096


def round_up(v, m):
    return -(-int(v) // m) * m


def red_zone_bytes(shape, element_size):
    if len(shape) < 3:
        return PASS_BYTES
    return round_up(PASS_BYTES + int(np.prod(shape[2:])) * element_size, ALIGN)


def dense_strides(shape, layout):
    """the strides of a fresh tensor of `shape` in `layout` (taken from torch itself, size-1 dims included)"""
    if layout == "contiguous":
        return torch.empty(list(shape), device="meta").stride()
    assert layout == "channels_last" and len(shape) in (4, 5), (layout, shape)
    fmt = torch.channels_last if len(shape) == 4 else torch.channels_last_3d
    return torch.empty(list(shape), device="meta", memory_format=fmt).stride()


class Guarded:
    def __init__(self, shape, dtype, device, layout="contiguous", offset_bytes=0):
        self.shape, self.dtype, self.layout = tuple(int(s) for s in shape), dtype, layout
        es = torch.empty(0, dtype=dtype).element_size()
        assert 0 <= offset_bytes < ALIGN and offset_bytes % es == 0, (offset_bytes, es)
        self.nbytes = int(np.prod(self.shape)) * es
        self.red = red_zone_bytes(self.shape, es)
        self._raw = torch.empty(2 * self.red + self.nbytes + 2 * ALIGN, dtype=torch.uint8, device=device)
        lead = (-self._raw.data_ptr()) % ALIGN + offset_bytes
        self.buf = self._raw[lead:lead + 2 * self.red + self.nbytes]        # red zone | interior | red zone
        self._interior = self.buf[self.red:self.red + self.nbytes]
        self.t = self._interior.view(dtype).as_strided(self.shape, dense_strides(self.shape, layout))
        self.byte = None
        assert self.t.data_ptr() % ALIGN == offset_bytes and self.t.data_ptr() == self._interior.data_ptr()

    def zones(self):
        return self.buf[:self.red], self.buf[self.red + self.nbytes:]

    def paint(self, byte):
        self.byte = int(byte)
        for z in self.zones():
            z.fill_(self.byte)
        return self

    def load(self, tensor):
        """values into the interior (any layout of `tensor`; the interior keeps its own)"""
        assert tuple(tensor.shape) == self.shape, (tuple(tensor.shape), self.shape)
        self.t.copy_(tensor.to(self.dtype))
        return self

    def poison(self):
        self._interior.fill_(POISON)
        return self

    def interior_bytes(self):
        """a copy of the interior's bytes, in memory order"""
        return self._interior.clone()

    def dirty(self):
        """0-dim bool tensor on the buffer's device: some red-zone byte is not the painted one (no host synchronisation)"""
        lo, hi = self.zones()
        return (lo != self.byte).any() | (hi != self.byte).any()

    def assert_intact(self, what):
        assert self.byte is not None, "paint() first"
        bad = torch.nonzero(self.buf != self.byte).view(-1)
        bad = bad[(bad < self.red) | (bad >= self.red + self.nbytes)] - self.red
        if bad.numel():
            first, last = int(bad[0]), int(bad[-1])
            raise AssertionError("red zone of %r written: %d bytes, first at offset %d, last at offset %d relative to the interior "
                                 "(%d bytes, red zones of %d, painted 0x%02X); %r"
                                 % (what[0] if what else None, bad.numel(), first, last, self.nbytes, self.red, self.byte, what))


def same_values(got, want):
    """the project's bit-for-bit comparison (pooled16_cases.assert_bits: torch.equal on the values): integers bit for bit; floats
    equal as values, so NaN equals nothing and the two zeros equal each other"""
    return got.shape == want.shape and got.dtype == want.dtype and bool(torch.equal(got, want))


def _first_difference(got, want):
    g, w = got.reshape(-1), want.reshape(-1)
    at = torch.nonzero(~(g == w)).view(-1)
    i = int(at[0])
    return "%d of %d differ, first at %r: %r, expected %r" % (at.numel(), g.numel(), tuple(int(v) for v in np.unravel_index(i, tuple(got.shape))),
                                                             g[i].item(), w[i].item())


def run_guarded(call, inputs, outputs, expect, what, patterns=PATTERNS, raises=None):
    """call(): runs the kernel on the buffers' `.t` and returns its name.  inputs: [(name, Guarded, tensor to load)]; outputs:
    [(name, Guarded)]; expect: per output a tensor of its shape and dtype (on any device), or None for an output whose content is
    unspecified (a workspace).  raises: a substring of the RuntimeError the call must end with instead -- then nothing may have been
    launched: every output keeps its poison.  -> the kernel name (the same under every pattern), or None with `raises`."""
    assert len(expect) == len(outputs)
    name, runs = None, []
    for byte in patterns:
        everything = [(n, g) for n, g, _ in inputs] + list(outputs)
        for _, g in everything:
            g.paint(byte)
        loaded = []
        for n, g, value in inputs:
            g.load(value)
            loaded.append(g.interior_bytes())
        for _, g in outputs:
            g.poison()
        if raises is None:
            kernel = call()
        else:
            kernel = None
            try:
                call()
            except RuntimeError as e:
                assert raises in str(e), what + (str(e),)
            else:
                raise AssertionError("did not raise %r: %r" % (raises, what))
        if everything[0][1].t.is_cuda:
            torch.cuda.synchronize()
        tag = what + (kernel, "pattern 0x%02X" % byte)
        # 1. every red zone, the inputs' included (one host round trip unless something is wrong)
        if bool(torch.stack([g.dirty() for _, g in everything]).any()):
            for n, g in everything:
                g.assert_intact((n,) + tag)
        # 2. inputs unchanged
        for (n, g, _), before in zip(inputs, loaded):
            assert torch.equal(g.interior_bytes(), before), ("input written", n) + tag
        # 3. outputs
        got = []
        for (n, g), want in zip(outputs, expect):
            if raises is not None:
                assert bool((g.interior_bytes() == POISON).all()), ("written by a refused call", n) + tag
                continue
            if want is None:
                continue
            have = g.t.cpu()
            want = want.cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
            assert have.shape == want.shape and have.dtype == want.dtype, (n, have.shape, want.shape, have.dtype, want.dtype) + tag
            assert same_values(have, want), (n, _first_difference(have, want)) + tag
            got.append((n, g.interior_bytes().cpu()))
        assert name is None or name == kernel, ("the patterns ran different kernels", name, kernel) + what
        name = kernel
        runs.append(got)
    for other in runs[1:]:
        for (n, a), (_, b) in zip(runs[0], other):
            assert torch.equal(a, b), ("outputs differ between the patterns", n, name) + what
    return name
