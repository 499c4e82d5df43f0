#!/usr/bin/env python3
"""Generate tests/golden/qtemporal.npz from the REAL reference: the expected int_repr of the quantized temporal shift.

Runs only where the reference build exists: like make_golden.py it loads oracle/_ref/_C.so (the reference's own QuantizedCPU
ops, built by oracle/build_ref.sh) and records inputs + outputs.  The fixture is data; no reference source travels.

    bash oracle/build_ref.sh && python tests/golden/make_golden_qtemporal.py

The reference has no temporal shift.  What is recorded is what the op is defined as: the reference's quantized shift2d of the
contiguous [N, C, T, M] copy of a [N*T, C, M] tensor under quint8 (zero point 128) weights (s_c, 0), permuted back to [N*T, C, M].

Grid: quint8 / qint8 / qint32 inputs with non-zero zero points x 5 paddings x T in (3, 4); each table holds 0, +1, -1, an entry
with |s| >= T and one with |s| >= 2 T.
  x_<dtype>_T<T>        int_repr of the input, [N*T, C, M]
  zp_<dtype>            its zero point
  shifts_T<T>           the table, int64 [C]
  out_<dtype>_T<T>_p<pad>   int_repr of the result, [N*T, C, M]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "_C.so")

torch.set_num_threads(1)
torch.ops.load_library(REF_SO)
OPS = torch.ops.torchshifts

N, C, M = 2, 6, 3
TABLES = {3: [0, 1, -1, 3, -7, 2], 4: [0, 1, -1, -4, 9, 2]}
QDT = {"quint8": (torch.quint8, torch.uint8, 0, 255, 7), "qint8": (torch.qint8, torch.int8, -128, 127, -3),
       "qint32": (torch.qint32, torch.int32, -100000, 100000, 11)}
SCALE = 0.05


def main():
    rs = np.random.RandomState(2718)
    d = {}
    for T, table in TABLES.items():
        d["shifts_T%d" % T] = np.array(table, np.int64)
        w = torch.zeros(C, 2)
        w[:, 0] = torch.tensor(table, dtype=torch.float32)
        wq = torch.quantize_per_tensor(w, 1.0, 128, torch.quint8)
        assert (wq.int_repr().long() - 128)[:, 0].tolist() == table
        for name, (qdt, idt, lo, hi, zp) in QDT.items():
            xi = rs.randint(lo, hi + 1, size=(N * T, C, M))
            d["x_%s_T%d" % (name, T)] = xi.astype({torch.uint8: np.uint8, torch.int8: np.int8, torch.int32: np.int32}[idt])
            d["zp_%s" % name] = np.array(zp)
            x = torch.from_numpy(xi).to(idt)
            view = x.view(N, T, C, M).permute(0, 2, 1, 3).contiguous()   # [N, C, T, M]
            xq = torch._make_per_tensor_quantized_tensor(view, SCALE, zp)
            for pad in range(5):
                out = OPS.shift2d(xq, wq, torch.Tensor(), pad, False)
                assert out.q_zero_point() == zp and abs(out.q_scale() - SCALE) < 1e-9
                back = out.int_repr().permute(0, 2, 1, 3).contiguous().view(N * T, C, M)
                d["out_%s_T%d_p%d" % (name, T, pad)] = back.numpy()
    path = os.path.join(HERE, "qtemporal.npz")
    np.savez_compressed(path, **d)
    print("%-16s %4d arrays %8.1f KB" % (os.path.basename(path), len(d), os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    sys.exit(main())
