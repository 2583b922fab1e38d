"""The NOAA HRPT tail on the GPU: HrptDemux, TipDemux and HirsDemux (include/qdsp_hip.h: NOAA HRPT, TIP and HIRS demultiplexers),
on the per-row operators' plumbing of qdsp_amd.ops.  A Deframer(110900) row feeds HrptDemux, its TIP rows and device counts feed
TipDemux, and HirsDemux(packet_stride=TipDemux.RECORD) reads the records in place: no host synchronisation in between.  There is
no fallback: the work runs in the kernels of csrc/noaa.hip or raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .ops import _Counts, _in_counts_ptr, _is_torch, _RowOp

__all__ = ["HrptDemux", "TipDemux", "HirsDemux"]


def _counts_arg(t, nchan, device):
    """(tensor, pointer) of an int32 count tensor: None makes one, False stands for a null pointer."""
    import torch

    if t is False:
        return None, None
    if t is None:
        t = torch.empty(nchan, dtype=torch.int32, device=device)
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == nchan
    return t, t.data_ptr()


class _Noaa(_Counts, _RowOp):
    _np = np.uint8
    _takes_in_counts = True

    def _setup(self, nchan, device):
        _RowOp.__init__(self)
        self.device = device
        self.nchan = int(nchan)

    def _whole(self, nbytes: int, item: int) -> int:
        if nbytes % item:
            raise ValueError(f"whole items of {item} bytes, not {nbytes} bytes")
        return nbytes // item

    def reset(self):
        pass                                      # no state between items


class HrptDemux(_Noaa):
    """dsp::noaa::HRPTDemux (src/dsp/noaa/hrpt.h): frames of 13863 bytes become five AVHRR image lines of 2048 uint16 and, by the
    frame's `minor` field, five TIP or five AIP minor frames of 104 bytes.  numpy input (whole frames, one row): the host entry
    point; a 1-D tensor: *_process_dev; both return (avhrr (5, n, 2048), tip (k, 104), aip (k, 104)), tip and aip as numpy arrays
    read back from the library's own rows.  A 2-D tensor of `nchan` rows: `process_batch`."""

    _prefix = "qdsp_hip_hrpt"
    _out_np = np.uint16
    FRAME, PIXELS, PLANES, MINOR, MINOR_PER_FRAME = 13863, 2048, 5, 104, 5

    def __init__(self, nchan: int = 1, device: int = 0, max_block: int = 64):
        self._setup(nchan, device)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, int(max_block)), "qdsp_hip_hrpt_create")

    def counts(self) -> np.ndarray:
        """(3, nchan): lines, TIP minor frames and AIP minor frames per row of the last call (synchronises the device)."""
        c = np.zeros((3, self.nchan), dtype=np.int32)
        capi.check(self._fn("get_counts")(self._h, c.ctypes.data_as(C.POINTER(C.c_int))))
        return c

    def _own(self, which: str, chan: int, cap: int) -> np.ndarray:
        y = np.empty((max(cap, 1), self.MINOR), np.uint8)
        n = capi.check(self._fn("get_" + which)(self._h, int(chan), y.ctypes.data, int(cap)), f"qdsp_hip_hrpt_get_{which}")
        return y[:min(n, cap)]

    def tip(self, chan: int = 0, cap: int = None) -> np.ndarray:
        """The TIP minor frames of row `chan` the last single-output call left on the device (synchronises)."""
        return self._own("tip", chan, int(self.counts()[1, chan]) if cap is None else cap)

    def aip(self, chan: int = 0, cap: int = None) -> np.ndarray:
        return self._own("aip", chan, int(self.counts()[2, chan]) if cap is None else cap)

    def own_dev(self, which: str):
        """(pointer, row stride in bytes, pointer of the int32 device counts) of the library's own "tip" or "aip" rows."""
        p, s, c = C.c_void_p(), C.c_int64(), C.c_void_p()
        capi.check(self._fn(which + "_dev")(self._h, C.byref(p), C.byref(s), C.byref(c)), f"qdsp_hip_hrpt_{which}_dev")
        return p.value, int(s.value), c.value

    def process(self, x, out=None):
        if _is_torch(x):
            return self.process_batch(x, avhrr=out) if x.dim() == 2 else self._process_dev(x, out)
        a = np.ascontiguousarray(x, dtype=np.uint8).ravel()
        n = self._whole(a.size, self.FRAME)
        y = np.empty((self.PLANES, max(n, 1), self.PIXELS), np.uint16)
        capi.check(self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data), "qdsp_hip_hrpt_process")
        if n == 0:
            return y[:, :0], np.empty((0, self.MINOR), np.uint8), np.empty((0, self.MINOR), np.uint8)
        return y, self.tip(0, 5 * n), self.aip(0, 5 * n)

    def _process_dev(self, x, out=None):
        import torch

        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.uint8 and x.dim() == 1 and self.nchan == 1, "one contiguous row"
        n = self._whole(x.numel(), self.FRAME)
        if out is None:
            out = torch.empty((self.PLANES, max(n, 1), self.PIXELS), dtype=torch.uint16, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint16 and out.numel() >= n * self.PLANES * self.PIXELS
        stream = torch.cuda.current_stream(x.device).cuda_stream
        capi.check(int(self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)), "qdsp_hip_hrpt_process_dev")
        if n == 0:
            return out[:, :0], np.empty((0, self.MINOR), np.uint8), np.empty((0, self.MINOR), np.uint8)
        return out.reshape(-1)[:self.PLANES * n * self.PIXELS].view(self.PLANES, n, self.PIXELS), self.tip(0, 5 * n), self.aip(0, 5 * n)

    def process_batch(self, x, nframes: int = None, in_counts=None, avhrr=None, tip=None, aip=None, tip_counts=None, aip_counts=None):
        """Channel c = row c of the 2-D uint8 tensor `x`, frames back to back (rows may be padded and begin at any byte).
        `in_counts`: an int32 device tensor of per-row frame counts (what Deframer.process_batch returns).  `avhrr`: a uint16
        tensor (nchan, 5, >= nframes, 2048) whose last dimension is contiguous, any row and plane strides; `tip` / `aip`: uint8
        tensors (nchan, >= nframes * 520).  None makes the output, False skips it (a null pointer).  Returns
        (avhrr, tip, tip_counts, aip, aip_counts), counts in minor frames as int32 device tensors.  Asynchronous."""
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.shape[0] == self.nchan and (x.shape[1] <= 1 or x.stride(1) == 1)
        n = x.shape[1] // self.FRAME if nframes is None else int(nframes)
        assert 0 <= n * self.FRAME <= x.shape[1]
        ap = rs = ps = None
        if avhrr is None:
            avhrr = torch.empty((self.nchan, self.PLANES, max(n, 1), self.PIXELS), dtype=torch.uint16, device=x.device)
        if avhrr is not False:
            assert avhrr.is_cuda and avhrr.dtype == torch.uint16 and avhrr.dim() == 4 and tuple(avhrr.shape[:2]) == (self.nchan, self.PLANES)
            assert avhrr.shape[2] >= n and avhrr.shape[3] == self.PIXELS and avhrr.stride(3) == 1 and (avhrr.shape[2] <= 1 or avhrr.stride(2) == self.PIXELS)
            ap, rs, ps = avhrr.data_ptr(), avhrr.stride(0), avhrr.stride(1)
        rows = []
        for t in (tip, aip):
            if t is None:
                t = torch.empty((self.nchan, max(n, 1) * 5 * self.MINOR), dtype=torch.uint8, device=x.device)
            if t is not False:
                assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[0] == self.nchan and t.shape[1] >= n * 5 * self.MINOR
                assert t.shape[1] <= 1 or t.stride(1) == 1
            rows.append(t)
        tip, aip = rows
        tc, tcp = _counts_arg(tip_counts, self.nchan, x.device)
        ac, acp = _counts_arg(aip_counts, self.nchan, x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = self._fn("process_batch_dev")(self._h, x.data_ptr(), n, x.stride(0), _in_counts_ptr(in_counts, self.nchan, x.device), ap, rs or 0,
                                           ps or 0, None if tip is False else tip.data_ptr(), 0 if tip is False else tip.stride(0), tcp,
                                           None if aip is False else aip.data_ptr(), 0 if aip is False else aip.stride(0), acp, stream)
        capi.check(int(rc), "qdsp_hip_hrpt_process_batch_dev")
        return (None if avhrr is False else avhrr[:, :, :n], None if tip is False else tip[:, :n * 5 * self.MINOR], tc,
                None if aip is False else aip[:, :n * 5 * self.MINOR], ac)

    def _time_count(self, x) -> int:
        return x.numel() // self.nchan // self.FRAME


class TipDemux(_Noaa):
    """dsp::noaa::TIPDemux (src/dsp/noaa/tip.h:31-124): every 104-byte minor frame becomes one record of RECORD bytes,
    HIRS[36] | SEM[2] | DCS[32] | SBUV[4]; `split` gives the four sections as strided views.  numpy input (whole minor frames,
    one row): the host entry point; a 1-D tensor: *_process_dev; both return (n, RECORD).  2-D: `process_batch`."""

    _prefix = "qdsp_hip_tip"
    _out_np = np.uint8
    FRAME = 104
    RECORD = 74
    HIRS, SEM, DCS, SBUV = 0, 36, 38, 70          # the sections' offsets in a record

    def __init__(self, nchan: int = 1, device: int = 0, max_block: int = 4096):
        self._setup(nchan, device)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, int(max_block)), "qdsp_hip_tip_create")

    @classmethod
    def split(cls, rec):
        """(hirs, sem, dcs, sbuv): views of the records' sections; `rec` is (..., RECORD)."""
        assert rec.shape[-1] == cls.RECORD
        return rec[..., cls.HIRS:cls.SEM], rec[..., cls.SEM:cls.DCS], rec[..., cls.DCS:cls.SBUV], rec[..., cls.SBUV:cls.RECORD]

    def process(self, x, out=None):
        if _is_torch(x):
            return self.process_batch(x, out) if x.dim() == 2 else self._process_dev(x, out)
        a = np.ascontiguousarray(x, dtype=np.uint8).ravel()
        n = self._whole(a.size, self.FRAME)
        y = np.empty((max(n, 1), self.RECORD), np.uint8)
        capi.check(self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data), "qdsp_hip_tip_process")
        return y[:n]

    def _process_dev(self, x, out=None):
        import torch

        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.uint8 and x.dim() == 1 and self.nchan == 1, "one contiguous row"
        n = self._whole(x.numel(), self.FRAME)
        if out is None:
            out = torch.empty(max(n, 1) * self.RECORD, dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= n * self.RECORD
        stream = torch.cuda.current_stream(x.device).cuda_stream
        capi.check(int(self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)), "qdsp_hip_tip_process_dev")
        return out.reshape(-1)[:n * self.RECORD].view(n, self.RECORD)

    def process_batch(self, x, out=None, count: int = None, in_counts=None, counts=None):
        """Channel c = row c of the 2-D uint8 tensor `x`, minor frames back to back (rows may be padded and begin at any byte).
        `in_counts`: per-row counts in minor frames (HrptDemux's tip_counts).  Returns (rows, counts): the (nchan, count * RECORD)
        view of `out` and the rows' counts as an int32 device tensor.  Asynchronous; `out` may not overlap `x`."""
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.shape[0] == self.nchan and (x.shape[1] <= 1 or x.stride(1) == 1)
        n = x.shape[1] // self.FRAME if count is None else int(count)
        assert 0 <= n * self.FRAME <= x.shape[1]
        if out is None:
            out = torch.empty((self.nchan, max(n, 1) * self.RECORD), dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == self.nchan and out.shape[1] >= n * self.RECORD
        assert out.shape[1] <= 1 or out.stride(1) == 1
        counts, cp = _counts_arg(counts, self.nchan, x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = self._fn("process_batch_dev")(self._h, x.data_ptr(), n, x.stride(0), _in_counts_ptr(in_counts, self.nchan, x.device), out.data_ptr(),
                                           out.stride(0), cp, stream)
        capi.check(int(rc), "qdsp_hip_tip_process_batch_dev")
        return out[:, :n * self.RECORD], counts

    def _time_count(self, x) -> int:
        return x.numel() // self.nchan // self.FRAME


class HirsDemux(_Noaa):
    """dsp::noaa::HIRSDemux (src/dsp/noaa/tip.h:136-238): 36-byte packets, `packet_stride` bytes apart, become scan lines of 56
    values in 20 radiance channels; a row carries lastElement, newImageData and the line in progress from call to call.  A call
    of n packets emits at most out_size(n) = n + 1 lines per row.  numpy input (one row of n * packet_stride bytes): the host
    entry point; a 1-D tensor: *_process_dev; both return (20, lines, 56) uint16.  2-D: `process_batch`."""

    _prefix = "qdsp_hip_hirs"
    _out_np = np.uint16
    PACKET, CHANNELS, LINE = 36, 20, 56

    def __init__(self, packet_stride: int = 36, nchan: int = 1, device: int = 0, max_block: int = 4096):
        packet_stride = int(packet_stride)
        if not self.PACKET <= packet_stride <= 4096:
            raise ValueError(f"packet_stride: 36 .. 4096, not {packet_stride}")
        self._setup(nchan, device)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, int(max_block), packet_stride), "qdsp_hip_hirs_create")
        self.packet_stride = packet_stride

    def reset(self):
        capi.check(self._fn("reset")(self._h), "qdsp_hip_hirs_reset")

    def get_state(self, chan: int = 0):
        """(lastElement, newImageData) of one row (synchronises the device)."""
        e, f = C.c_int(), C.c_int()
        capi.check(self._fn("get_state")(self._h, int(chan), C.byref(e), C.byref(f)), "qdsp_hip_hirs_get_state")
        return int(e.value), bool(f.value)

    def set_state(self, last_element: int, new_image_data: bool, chan: int = -1):
        capi.check(self._fn("set_state")(self._h, int(chan), int(last_element), int(bool(new_image_data))), "qdsp_hip_hirs_set_state")

    def process(self, x, out=None):
        if _is_torch(x):
            return self.process_batch(x, out) if x.dim() == 2 else self._process_dev(x, out)
        a = np.ascontiguousarray(x, dtype=np.uint8).ravel()
        n = self._whole(a.size, self.packet_stride)
        y = np.empty((self.CHANNELS, n + 1, self.LINE), np.uint16)
        lines = capi.check(self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data), "qdsp_hip_hirs_process")
        return y[:, :lines]

    def _process_dev(self, x, out=None):
        import torch

        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.uint8 and x.dim() == 1 and self.nchan == 1, "one contiguous row"
        n = self._whole(x.numel(), self.packet_stride)
        if out is None:
            out = torch.empty((self.CHANNELS, n + 1, self.LINE), dtype=torch.uint16, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint16 and out.numel() >= self.CHANNELS * (n + 1) * self.LINE
        stream = torch.cuda.current_stream(x.device).cuda_stream
        capi.check(int(self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)), "qdsp_hip_hirs_process_dev")
        lines = int(self.counts()[0]) if n else 0
        return out.reshape(-1)[:self.CHANNELS * (n + 1) * self.LINE].view(self.CHANNELS, n + 1, self.LINE)[:, :lines]

    def process_batch(self, x, out=None, count: int = None, in_counts=None, counts=None):
        """Channel c = row c of the 2-D uint8 tensor `x`, packets packet_stride bytes apart (rows may be padded and begin at any
        byte).  `in_counts`: per-row packet counts (TipDemux's counts).  `out`: a uint16 tensor (nchan, 20, >= count + 1, 56) whose
        last two dimensions are contiguous, any row and plane strides.  Returns (lines, counts): the (nchan, 20, count + 1, 56) view
        of `out`, row c's first counts[c] lines written and the rest untouched, and the line counts as an int32 device tensor."""
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.shape[0] == self.nchan and (x.shape[1] <= 1 or x.stride(1) == 1)
        n = x.shape[1] // self.packet_stride if count is None else int(count)
        assert n == 0 or (n - 1) * self.packet_stride + self.PACKET <= x.shape[1]
        if out is None:
            out = torch.empty((self.nchan, self.CHANNELS, n + 1, self.LINE), dtype=torch.uint16, device=x.device)
        assert out.is_cuda and out.dtype == torch.uint16 and out.dim() == 4 and tuple(out.shape[:2]) == (self.nchan, self.CHANNELS)
        assert out.shape[2] >= n + 1 and out.shape[3] == self.LINE and out.stride(3) == 1 and out.stride(2) == self.LINE
        counts, cp = _counts_arg(counts, self.nchan, x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = self._fn("process_batch_dev")(self._h, x.data_ptr(), n, x.stride(0), _in_counts_ptr(in_counts, self.nchan, x.device), out.data_ptr(),
                                           out.stride(0), out.stride(1), cp, stream)
        capi.check(int(rc), "qdsp_hip_hirs_process_batch_dev")
        return out[:, :, :n + 1], counts

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per call of `iters` back-to-back process_batch calls over the rows of the 2-D tensor `x`.  The state moves on."""
        import torch

        counts = torch.empty(self.nchan, dtype=torch.int32, device=x.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(int(iters)):
            self.process_batch(x, out, counts=counts)
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1)) / int(iters)
