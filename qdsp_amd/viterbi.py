"""The Viterbi decoder of libcorrect's convolutional codes on the GPU (include/qdsp_hip.h: Viterbi decoder), batched over channel
rows x terminated frames.  Every count here is in frames.  The decoder keeps nothing between calls; its handle is known to the
library by its address, in a set of its own.  There is no fallback: the decode runs in viterbi_decode_kernel or raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ops import _in_counts_ptr, _is_torch

__all__ = ["ViterbiDecoder", "Viterbi27"]


class ViterbiDecoder:
    """correct_convolutional_decode_soft (soft=True: uint8 symbols, 0 a strong zero, 255 a strong one) or correct_convolutional_decode
    (soft=False: packed bits, MSB first) of a freshly created correct_convolutional(rate, order, poly), bit for bit, on frames of
    `sets` groups of `rate` symbols: frame_in_bytes in, frame_out_bytes = (sets - order + 1) // 8 out.  rate 2 or 3, order 6 .. 9,
    polynomials below 2^order, order + 7 <= sets <= 65536.  numpy input (whole frames, one row): the host entry point, returns
    (frames, frame_out_bytes); a 1-D tensor: *_process_dev; a 2-D tensor of `nchan` rows: `process_batch`."""

    _prefix = "qdsp_hip_viterbi"

    def __init__(self, rate: int, order: int, poly, sets: int, soft: bool = True, nchan: int = 1, max_block: int = 4096, device: int = 0):
        rate, order, sets = int(rate), int(order), int(sets)
        if rate not in (2, 3):
            raise ValueError(f"rate: 2 or 3, not {rate}")
        if not 6 <= order <= 9:
            raise ValueError(f"order: 6 .. 9, not {order}")
        p = [int(v) for v in poly]
        if len(p) != rate or any(not 0 <= v < (1 << order) for v in p):
            raise ValueError(f"poly: {rate} polynomials below 2^{order}, not {poly!r}")
        if not order + 7 <= sets <= 65536:
            raise ValueError(f"sets: {order + 7} .. 65536, not {sets}")
        self._L = capi.load()
        self._h = C.c_void_p()
        self.device, self.nchan = int(device), int(nchan)
        self.rate, self.order, self.poly, self.sets, self.soft = rate, order, tuple(p), sets, bool(soft)
        pa = (C.c_uint16 * rate)(*p)
        rc = self._fn("create")(C.byref(self._h), self.device, self.nchan, int(max_block), rate, order, pa, sets, int(self.soft))
        capi.check(rc, "qdsp_hip_viterbi_create")
        self.frame_in_bytes = int(self._fn("frame_in_bytes")(self._h))
        self.frame_out_bytes = int(self._fn("frame_out_bytes")(self._h))

    def _fn(self, name):
        return getattr(self._L, f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def last_kernel(self):
        name = C.create_string_buffer(128)
        g, b, l = C.c_int(), C.c_int(), C.c_int()
        capi.check(self._L.qdsp_hip_last_kernel(self._h, name, 128, C.byref(g), C.byref(b), C.byref(l)))
        return {"name": name.value.decode(), "grid": g.value, "block": b.value, "lds_bytes": l.value}

    def _whole_frames(self, nbytes: int) -> int:
        if nbytes % self.frame_in_bytes:
            raise ValueError(f"whole frames of {self.frame_in_bytes} bytes, not {nbytes} bytes")
        return nbytes // self.frame_in_bytes

    def process(self, x, out=None):
        if _is_torch(x):
            return self.process_batch(x, out) if x.dim() == 2 else self._process_dev(x, out)
        a = np.ascontiguousarray(x, dtype=np.uint8).ravel()
        n = self._whole_frames(a.size)
        y = np.empty(max(n, 1) * self.frame_out_bytes, np.uint8)
        capi.check(self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data), "qdsp_hip_viterbi_process")
        return y[:n * self.frame_out_bytes].reshape(n, self.frame_out_bytes)

    def _process_dev(self, x, out=None):
        import torch

        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.uint8 and x.dim() == 1 and self.nchan == 1, "one contiguous row"
        n = self._whole_frames(x.numel())
        if out is None:
            out = torch.empty(max(n, 1) * self.frame_out_bytes, dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= n * self.frame_out_bytes
        stream = torch.cuda.current_stream(x.device).cuda_stream
        capi.check(int(self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)), "qdsp_hip_viterbi_process_dev")
        return out[:n * self.frame_out_bytes].reshape(n, self.frame_out_bytes)

    def process_batch(self, d_in, nframes: int = None, d_in_counts=None, out=None):
        """Channel c = row c of the 2-D uint8 tensor `d_in`, frames back to back (rows may be padded and start at any byte).
        `d_in_counts`: an int32 device tensor of per-row frame counts (what Deframer.process_batch returns); frames behind a row's
        count leave their output untouched.  Returns the (nchan, nframes * frame_out_bytes) view of `out`, or of new rows.
        Asynchronous, on torch's current stream; `out` may not overlap `d_in`."""
        import torch

        x = d_in
        assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.shape[0] == self.nchan and (x.shape[1] <= 1 or x.stride(1) == 1)
        n = x.shape[1] // self.frame_in_bytes if nframes is None else int(nframes)
        assert 0 <= n * self.frame_in_bytes <= x.shape[1]
        if out is None:
            out = torch.empty((self.nchan, max(n, 1) * self.frame_out_bytes), dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == self.nchan
        assert out.shape[1] >= n * self.frame_out_bytes and (out.shape[1] <= 1 or out.stride(1) == 1)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = self._fn("process_batch_dev")(self._h, x.data_ptr(), n, x.stride(0), _in_counts_ptr(d_in_counts, self.nchan, x.device), out.data_ptr(),
                                           out.stride(0), stream)
        capi.check(int(rc), "qdsp_hip_viterbi_process_batch_dev")
        return out[:, :n * self.frame_out_bytes]

    def process_ex(self, x, in_link: int, count: int, out, out_link: int):
        """The block-graph entry point on raw pointers (host or device, QDSP_HIP_LINK_* codes); one row."""
        return capi.check(self._fn("process_ex")(self._h, int(x), int(in_link), int(count), int(out), int(out_link)), "qdsp_hip_viterbi_process_ex")

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per call of `iters` back-to-back process_batch calls over the rows of the 2-D tensor `x`."""
        import torch

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(int(iters)):
            self.process_batch(x, out=out)
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1)) / int(iters)


class Viterbi27(ViterbiDecoder):
    """The rate-1/2, k = 7 code with polynomials (0161, 0127): libcorrect's correct_conv_r12_7_polynomial."""

    POLY = (0o161, 0o127)

    def __init__(self, sets: int, soft: bool = True, nchan: int = 1, max_block: int = 4096, device: int = 0):
        super().__init__(2, 7, self.POLY, sets, soft=soft, nchan=nchan, max_block=max_block, device=device)
