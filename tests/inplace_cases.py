"""What the in-place temporal shift tests share: the reference and the tables.

The reference is the definition in the README: the oracle's 2-D sparse forward (oracle.oracle, pinned to the reference) of the
[N, C, T, M] view under the table (s, 0), computed from a clone taken BEFORE the call under test.  The op is a pure gather, so the
oracle works on the tensor's bits: fp32 / fp64 tensors through its float forward (which rounds the table itself, half to even), every
other element type through its integer forward on the same bytes -- a 16-bit element as two uint8 columns of its plane, which a shift
along T moves together -- under the table the oracle's own weight conversion rounds."""
import numpy as np
import torch

from oracle import oracle as O

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
U8, I8, I32 = torch.uint8, torch.int8, torch.int32
PADS = (0, 1, 2, 3, 4)
INT_VIEW = {torch.quint8: U8, torch.qint8: I8, torch.qint32: I32}


def oracle_table(shifts):
    """the integers the reference makes of a table: [C] int64 (floats rounded half to even by the oracle's conversion)"""
    s = shifts.detach().cpu().reshape(-1)
    if not s.is_floating_point():
        return s.to(torch.int64).numpy()
    iw, _ = O.weights_forward(s.to(torch.float64).numpy().reshape(-1, 1), False)
    return iw.reshape(-1)


def reference(x, shifts, T, pad, zero_point=0):
    """x: a CPU tensor [N*T, C, ...] of a plain dtype (for a quantized tensor: its int_repr and its zero point), any strides.
    Returns the shifted tensor, contiguous, same dtype, bit for bit what the definition gives."""
    assert x.device.type == "cpu" and not x.is_quantized
    xc = x.detach().contiguous()
    NT, C = xc.shape[:2]
    N = NT // T
    s = oracle_table(shifts)
    if xc.numel() == 0:
        return xc.clone()
    if xc.dtype in (F32, F64):
        v = np.ascontiguousarray(xc.numpy().reshape(N, T, C, -1).transpose(0, 2, 1, 3))
        w = np.stack([s, np.zeros_like(s)], 1).astype(v.dtype)
        out = O.forward(v, w, pad, False)
    else:
        if xc.dtype in (U8, I8, I32):
            bits, fill = xc.numpy(), zero_point
        else:
            assert zero_point == 0
            bits, fill = xc.view(U8).numpy(), 0   # (the last dim in bytes)
        v = np.ascontiguousarray(bits.reshape(N, T, C, -1).transpose(0, 2, 1, 3))
        out = O.forward_q(v, np.stack([s, np.zeros_like(s)], 1), 0, fill, pad)
    out = torch.from_numpy(np.ascontiguousarray(out.transpose(0, 2, 1, 3)))
    if xc.dtype in (F16, BF16):
        return out.reshape(-1).view(xc.dtype).reshape(xc.shape)
    return out.reshape(xc.shape)


def same_bits(a, b):
    """bit-for-bit equality of two tensors of one dtype and shape (NaN payloads and signed zeros count)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.is_quantized:
        a, b = a.int_repr(), b.int_repr()
    return torch.equal(a.reshape(-1).view(U8), b.reshape(-1).view(U8))


def random_table(rs, C, T, dtype=torch.int64):
    """shifts from [-2T-1, 2T+1] with 0 and both ends always present where C allows"""
    s = rs.randint(-2 * T - 1, 2 * T + 2, size=C)
    s[[0, C // 2, C - 1][:C]] = [0, 2 * T + 1, -2 * T - 1][:C]
    return torch.from_numpy(s.astype(np.int64)).to(dtype)


def published_table(C, fold_div=8):
    s = torch.zeros(C, dtype=torch.int64)
    fold = C // fold_div
    s[:fold] = -1
    s[fold:2 * fold] = 1
    return s


def data(rs, shape, dtype):
    """random values of a float or integer dtype (integers: the whole range of one byte, +-10^6 for int32)"""
    if dtype in (U8, I8):
        lo = 0 if dtype == U8 else -128
        return torch.from_numpy(rs.randint(lo, lo + 256, size=shape)).to(dtype)
    if dtype == I32:
        return torch.from_numpy(rs.randint(-1000000, 1000000, size=shape)).to(dtype)
    return torch.from_numpy(rs.uniform(-1, 1, size=shape)).to(dtype)
