"""Guarded device buffers for the GPU tests that call the C ABI with raw pointers
(tests/test_gpu_xagg_edges.py, tests/test_gpu_gemm_edges.py)."""
import ctypes

import numpy as np
import torch

from xagg_ref import SENT32

DEV = "cuda"
f32 = np.float32


class Buf:
    """A rows x cols matrix inside a flat device buffer: 8 guard elements in front (the matrix stays
    16-byte aligned), rows ld >= cols apart, 8 guard elements behind; everything outside ``data`` holds
    ``fill``, a finite non-zero sentinel."""

    def __init__(self, rows, cols, dtype=f32, fill=SENT32, ld=None, data=None):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.lead = rows, cols, ld, 8
        host = np.full(8 + rows * ld + 8, fill, dtype)
        if data is not None:
            self._matrix(host)[:, :cols] = np.asarray(data, dtype).reshape(rows, cols)
        self.host = host
        self.dev = torch.from_numpy(host.copy()).to(DEV)
        self.addr = self.dev.data_ptr() + 8 * host.itemsize
        self.ptr = ctypes.c_void_p(self.addr)

    def _matrix(self, flat):
        return flat[self.lead:self.lead + self.rows * self.ld].reshape(self.rows, self.ld)

    def read(self):
        """(the matrix as it is now, whether every element outside it still has its first bits)."""
        got = self.dev.cpu().numpy()
        inner = self._matrix(got)[:, :self.cols].copy()
        was = self.host.copy()
        self._matrix(got)[:, :self.cols] = 0
        self._matrix(was)[:, :self.cols] = 0
        return inner, bool(np.array_equal(got.view(np.uint8), was.view(np.uint8)))

    def untouched(self):
        return bool(np.array_equal(self.dev.cpu().numpy().view(np.uint8), self.host.view(np.uint8)))
