"""The Falcon 9 tail on the GPU: FalconPacketSync (include/qdsp_hip.h: FalconPacketSync), on the per-row operators' plumbing of
qdsp_amd.ops.  A Deframer row feeds fec.FalconRs, and FalconPacketSync(frame_stride=1275) reads its frames and device counts in
place: no host synchronisation in between.  There is no fallback: the work runs in the kernels of csrc/fpkt.hip or raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ops import _Counts, _in_counts_ptr, _is_torch, _RowOp

__all__ = ["FalconPacketSync"]


class FalconPacketSync(_Counts, _RowOp):
    """dsp::FalconPacketSync (src/dsp/falcon_packet.h): frames, `frame_stride` bytes apart, of a 4-byte header and 1191 data bytes
    become the packets the headers delimit; a row carries lastCounter, packetRead and the pending packet from call to call.  A
    call of n frames emits at most out_packets(n) = 398 n packets in at most out_size(n) = 16392 + 1191 n bytes per row.  numpy
    input (one row of n * frame_stride bytes): the host entry point; a 1-D tensor: *_process_dev; both return the packets as a
    list of `bytes` (with_offs=True: the row's bytes and its offsets instead).  2-D: `process_batch`."""

    _prefix = "qdsp_hip_fpkt"
    _np = np.uint8
    _out_np = np.uint8
    _takes_in_counts = True
    FRAME, DATA, MAX_PACKET, PER_FRAME = 1195, 1191, 16392, 398

    def __init__(self, frame_stride: int = 1275, nchan: int = 1, device: int = 0, max_block: int = 4096):
        frame_stride = int(frame_stride)
        if not self.FRAME <= frame_stride <= 4096:
            raise ValueError(f"frame_stride: 1195 .. 4096, not {frame_stride}")
        _RowOp.__init__(self)
        self.device = device
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, int(max_block), frame_stride), "qdsp_hip_fpkt_create")
        self.frame_stride = frame_stride

    def _whole(self, nbytes: int) -> int:
        if nbytes % self.frame_stride:
            raise ValueError(f"whole frames of {self.frame_stride} bytes, not {nbytes} bytes")
        return nbytes // self.frame_stride

    def out_packets(self, n: int) -> int:
        """The most packets per row a call of `n` frames per row can emit: an offset row needs one entry more."""
        return int(capi.check(int(self._fn("out_packets")(self._h, int(n))), "qdsp_hip_fpkt_out_packets"))

    def counts(self) -> np.ndarray:
        """(2, nchan): packets and bytes per row of the last call (synchronises the device)."""
        c = np.zeros((2, self.nchan), dtype=np.int32)
        capi.check(self._fn("get_counts")(self._h, c.ctypes.data_as(C.POINTER(C.c_int))))
        return c

    def offsets(self, chan: int = 0, cap: int = None) -> np.ndarray:
        """The offsets (count + 1 entries) of row `chan` in the library's own table, which the single-row forms and a batch call
        without `offs` fill (synchronises the device)."""
        if cap is None:
            cap = int(self.counts()[0, chan])
        o = np.zeros(cap + 1, np.int32)
        n = capi.check(self._fn("get_offsets")(self._h, int(chan), o.ctypes.data, int(cap)), "qdsp_hip_fpkt_get_offsets")
        return o[:min(n, cap) + 1]

    def offs_dev(self):
        """(pointer, row stride in entries, pointer of the int32 [2][nchan] device counts) of the library's own offset table."""
        p, s, c = C.c_void_p(), C.c_int64(), C.c_void_p()
        capi.check(self._fn("offs_dev")(self._h, C.byref(p), C.byref(s), C.byref(c)), "qdsp_hip_fpkt_offs_dev")
        return p.value, int(s.value), c.value

    @staticmethod
    def packets(out_row, offs_row, count: int) -> list:
        """The first `count` packets of a row as `bytes`: `out_row` the row's bytes, `offs_row` its offsets (count + 1 used)."""
        if _is_torch(out_row):
            out_row = out_row.cpu().numpy()
        if _is_torch(offs_row):
            offs_row = offs_row.cpu().numpy()
        o = np.asarray(offs_row)[:int(count) + 1].astype(np.int64)
        buf = np.ascontiguousarray(out_row, dtype=np.uint8)[:int(o[-1]) if len(o) else 0].tobytes()
        return [buf[int(o[k]):int(o[k + 1])] for k in range(int(count))]

    def get_state(self, chan: int = 0):
        """(lastCounter, packetRead, the pending bytes) of one row (synchronises the device)."""
        ctr, rd = C.c_uint32(), C.c_int()
        pend = np.zeros(self.MAX_PACKET, np.uint8)
        capi.check(self._fn("get_state")(self._h, int(chan), C.byref(ctr), C.byref(rd), pend.ctypes.data), "qdsp_hip_fpkt_get_state")
        return int(ctr.value), int(rd.value), pend[:max(int(rd.value), 0)].tobytes()

    def set_state(self, last_counter: int, pending: bytes = None, chan: int = -1):
        """lastCounter and the pending packet (None or empty: nothing pending) of one row or, chan -1, of all."""
        p = np.frombuffer(bytes(pending or b""), np.uint8)
        if p.size > self.MAX_PACKET:
            raise ValueError(f"pending: at most {self.MAX_PACKET} bytes, not {p.size}")
        rc = self._fn("set_state")(self._h, int(chan), int(last_counter) & 0xFFFFFFFF, p.size if p.size else -1, p.ctypes.data if p.size else None)
        capi.check(rc, "qdsp_hip_fpkt_set_state")

    def process(self, x, out=None, with_offs: bool = False):
        if _is_torch(x):
            return self.process_batch(x, out) if x.dim() == 2 else self._process_dev(x, out, with_offs)
        a = np.ascontiguousarray(x, dtype=np.uint8).ravel()
        n = self._whole(a.size)
        y = np.empty(self.out_size(n), np.uint8)
        count = capi.check(self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data), "qdsp_hip_fpkt_process")
        offs = self.offsets(0, count) if n else np.zeros(1, np.int32)
        return (y[:int(offs[count])].tobytes(), offs) if with_offs else self.packets(y, offs, count)

    def _process_dev(self, x, out=None, with_offs: bool = False):
        import torch

        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.uint8 and x.dim() == 1 and self.nchan == 1, "one contiguous row"
        n = self._whole(x.numel())
        if out is None:
            out = torch.empty(self.out_size(n), dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= self.out_size(n)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        capi.check(int(self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)), "qdsp_hip_fpkt_process_dev")
        count = int(self.counts()[0, 0]) if n else 0
        offs = self.offsets(0, count) if n else np.zeros(1, np.int32)
        y = out[:int(offs[count])].cpu().numpy()
        return (y.tobytes(), offs) if with_offs else self.packets(y, offs, count)

    def process_batch(self, x, out=None, offs=None, nframes: int = None, in_counts=None, counts=None):
        """Channel c = row c of the 2-D uint8 tensor `x`, frames frame_stride bytes apart (rows may be padded and begin at any
        byte).  `in_counts`: an int32 device tensor of per-row frame counts (FalconRs's counts).  `out`: a uint8 tensor (nchan, >=
        out_size(nframes)); `offs`: an int32 tensor (nchan, >= out_packets(nframes) + 1), or False for the library's own table
        (`offsets`).  Returns (out, offs, counts): row c's counts[c] packets back to back in out[c], packet k at offs[c, k] ..
        offs[c, k + 1]; everything behind is untouched; counts an int32 device tensor.  Asynchronous; `out` may not overlap `x`."""
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.shape[0] == self.nchan and (x.shape[1] <= 1 or x.stride(1) == 1)
        n = x.shape[1] // self.frame_stride if nframes is None else int(nframes)
        assert n == 0 or (n - 1) * self.frame_stride + self.FRAME <= x.shape[1]
        nb, npk = self.out_size(n), self.out_packets(n)
        if out is None:
            out = torch.empty((self.nchan, nb), dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == self.nchan and out.shape[1] >= nb
        assert out.stride(1) == 1
        if offs is None:
            offs = torch.empty((self.nchan, npk + 1), dtype=torch.int32, device=x.device)
        op, ostride = None, 0
        if offs is not False:
            assert offs.is_cuda and offs.dtype == torch.int32 and offs.dim() == 2 and offs.shape[0] == self.nchan and offs.shape[1] >= npk + 1
            assert offs.stride(1) == 1
            op, ostride = offs.data_ptr(), offs.stride(0)
        if counts is None:
            counts = torch.empty(self.nchan, dtype=torch.int32, device=x.device)
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == self.nchan
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = self._fn("process_batch_dev")(self._h, x.data_ptr(), n, x.stride(0), _in_counts_ptr(in_counts, self.nchan, x.device), out.data_ptr(),
                                           out.stride(0), op, ostride, counts.data_ptr(), stream)
        capi.check(int(rc), "qdsp_hip_fpkt_process_batch_dev")
        return out[:, :nb], (None if offs is False else offs[:, :npk + 1]), counts

    def time_dev(self, x, out, iters: int, offs=None) -> float:
        """Mean ms per call of `iters` back-to-back process_batch calls over the rows of the 2-D tensor `x`.  The state moves on."""
        import torch

        n = x.shape[1] // self.frame_stride
        counts = torch.empty(self.nchan, dtype=torch.int32, device=x.device)
        if offs is None:
            offs = torch.empty((self.nchan, self.out_packets(n) + 1), dtype=torch.int32, device=x.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(int(iters)):
            self.process_batch(x, out, offs, counts=counts)
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1)) / int(iters)
