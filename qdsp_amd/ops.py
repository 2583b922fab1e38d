"""Operator-level front-end of the C ABI, one class per reference block on the hot path.

    Fir        <-> dsp::FIR<T>                 (src/dsp/filter.h:9-88)
    Resampler  <-> dsp::PolyphaseResampler<T>  (src/dsp/resampling.h:9-189)
    Xlator     <-> dsp::FrequencyXlator<T>     (src/dsp/processing.h:10-81)
    Vfo        <-> dsp::VFO                    (src/dsp/vfo.h), fused into one kernel

`process(x)`: a numpy array takes the host-pointer entry point (`*_process`, what a block's
run() calls on the stream buffers); a CUDA/HIP torch tensor takes `*_process_dev` on torch's
current stream.  One call == one run() of the reference block.  torch is only used for
device memory and streams.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

FL_M_PI = np.float32(3.1415926535)  # src/dsp/types.h:4


def phase_delta(sample_rate: float, freq: float):
    """phaseDelta exactly as FrequencyXlator::init computes it (processing.h:20): theta in
    float with FL_M_PI, then the float cos/sin overloads."""
    theta = np.float32(np.float32(np.float32(freq) / np.float32(sample_rate)) * np.float32(2.0)) * FL_M_PI
    return float(_libm().cosf(C.c_float(theta))), float(_libm().sinf(C.c_float(theta)))


_LIBM = None


def _libm():
    """glibc's cosf/sinf -- the same functions std::cos(float)/std::sin(float) resolve to in
    the C++ host code (numpy's float32 cos may differ in the last bit)."""
    global _LIBM
    if _LIBM is None:
        _LIBM = C.CDLL("libm.so.6")
        for f in (_LIBM.cosf, _LIBM.sinf):
            f.restype = C.c_float
            f.argtypes = [C.c_float]
    return _LIBM


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _taps_ptr(taps):
    t = np.ascontiguousarray(taps, dtype=np.float32)
    return t, t.ctypes.data_as(C.POINTER(C.c_float))


class _Op:
    _prefix = ""
    _ch = 2

    def __init__(self):
        self._L = capi.load()
        self._h = C.c_void_p()
        self.device = 0

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

    # -- data plumbing ---------------------------------------------------------------------
    def _np_in(self, x):
        a = np.ascontiguousarray(x)
        if self._ch == 2:
            if a.dtype != np.complex64:
                a = a.astype(np.complex64)
            return a, a.size
        return np.ascontiguousarray(a, dtype=np.float32), a.size

    def _out_size(self, n: int) -> int:
        return n

    def process(self, x, out=None):
        if _is_torch(x):
            return self._process_dev(x, out)
        a, n = self._np_in(x)
        no = self._out_size(n)
        y = np.empty(max(no, 1), dtype=np.complex64 if self._ch == 2 else np.float32)
        rc = self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data)
        capi.check(rc, self._prefix + "_process")
        return y[:no]

    def _process_dev(self, x, out=None):
        import torch

        assert x.is_cuda and x.is_contiguous()
        want = torch.complex64 if self._ch == 2 else torch.float32
        assert x.dtype == want, f"expected {want}"
        n = x.numel()
        no = self._out_size(n)
        if out is None:
            out = torch.empty(max(no, 1), dtype=want, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.numel() >= no and out.dtype == want
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)
        capi.check(int(rc), self._prefix + "_process_dev")
        return out[:no]

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per launch of `iters` back-to-back process_dev calls, HIP events on the
        launch stream (qdsp_hip_time_process_dev)."""
        import torch

        stream = torch.cuda.current_stream(x.device).cuda_stream
        ms = C.c_float()
        rc = self._L.qdsp_hip_time_process_dev(self._h, x.data_ptr(), x.numel(), out.data_ptr(), stream, iters, C.byref(ms))
        capi.check(rc, "qdsp_hip_time_process_dev")
        return float(ms.value)

    def last_kernel(self):
        name = C.create_string_buffer(128)
        g, b, l = C.c_int(), C.c_int(), C.c_int()
        capi.check(self._L.qdsp_hip_last_kernel(self._h, name, 128, C.byref(g), C.byref(b), C.byref(l)))
        return {"name": name.value.decode(), "grid": g.value, "block": b.value, "lds_bytes": l.value}


class _HistMixin:
    AUTO, DIRECT, FFT = 0, 1, 2

    def set_mode(self, mode: int):
        """AUTO / DIRECT (direct form) / FFT (overlap-save fast convolution), *_set_mode."""
        capi.check(self._fn("set_mode")(self._h, int(mode)))

    def reset(self):
        capi.check(self._fn("reset")(self._h))

    @property
    def history_len(self) -> int:
        return capi.check(self._fn("history_len")(self._h))

    def get_history(self) -> np.ndarray:
        n = self.history_len
        a = np.zeros(max(n, 1), dtype=np.complex64 if self._ch == 2 else np.float32)
        capi.check(self._fn("get_history")(self._h, a.ctypes.data))
        return a[:n]

    def set_history(self, hist):
        a, n = self._np_in(hist)
        assert n == self.history_len, (n, self.history_len)
        capi.check(self._fn("set_history")(self._h, a.ctypes.data))

    def history_dev_ptr(self) -> int:
        p = C.c_void_p()
        capi.check(self._fn("history_dev")(self._h, C.byref(p)))
        return p.value or 0

    def set_history_dev(self, t):
        """Device-to-device copy of `history_len` samples from torch tensor `t` into the history
        the next call reads, on torch's current stream (*_set_history_dev)."""
        import torch

        assert t.is_cuda and t.is_contiguous() and t.numel() == self.history_len
        stream = torch.cuda.current_stream(t.device).cuda_stream
        capi.check(self._fn("set_history_dev")(self._h, t.data_ptr(), stream))

    def set_history_ptr(self, ptr: int, stream: int):
        """The same from a raw device pointer (the receive buffer of the C ring, qdsp_hip_ring_complete) on HIP stream `stream`."""
        capi.check(self._fn("set_history_dev")(self._h, int(ptr), int(stream)))

    def history_dev_tensor(self):
        """The device history buffer the NEXT process call reads, as a torch view (no copy):
        an RCCL recv of the neighbour's tail can land here directly (multi-GPU halo)."""
        import torch

        n = self.history_len
        ptr = self.history_dev_ptr()
        nfloat = n * self._ch

        class _Holder:
            pass

        holder = _Holder()
        holder.__cuda_array_interface__ = {
            "shape": (nfloat,), "typestr": "<f4", "data": (ptr, False), "version": 2,
        }
        t = torch.as_tensor(holder, device=f"cuda:{self.device}")
        return torch.view_as_complex(t.view(n, 2)) if self._ch == 2 else t


class Fir(_Op, _HistMixin):
    def __init__(self, taps, complex_data: bool = True, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self._ch = 2 if complex_data else 1
        self._prefix = "qdsp_hip_fir_cf32" if complex_data else "qdsp_hip_fir_f32"
        self.device = device
        self._taps, p = _taps_ptr(taps)
        capi.check(self._fn("create")(C.byref(self._h), device, p, len(self._taps), max_block), self._prefix + "_create")

    def set_taps(self, taps):
        self._taps, p = _taps_ptr(taps)
        capi.check(self._fn("set_taps")(self._h, p, len(self._taps)))


class Resampler(_Op, _HistMixin):
    def __init__(self, taps, interp: int, decim: int, complex_data: bool = True, device: int = 0,
                 max_block: int = 1_000_000):
        super().__init__()
        self._ch = 2 if complex_data else 1
        self._prefix = "qdsp_hip_decim_cf32" if complex_data else "qdsp_hip_decim_f32"
        self.device = device
        self._taps, p = _taps_ptr(taps)
        capi.check(self._fn("create")(C.byref(self._h), device, p, len(self._taps), int(interp), int(decim), max_block),
                   self._prefix + "_create")

    def configure(self, taps, interp: int, decim: int):
        self._taps, p = _taps_ptr(taps)
        capi.check(self._fn("configure")(self._h, p, len(self._taps), int(interp), int(decim)))

    def _out_size(self, n: int) -> int:
        return int(capi.check(self._fn("out_size")(self._h, n)))


class _NcoMixin:
    def set_phase_inc(self, re: float, im: float):
        capi.check(self._fn("set_phase_inc")(self._h, re, im))

    def get_phase(self) -> complex:
        re, im = C.c_float(), C.c_float()
        capi.check(self._fn("get_phase")(self._h, C.byref(re), C.byref(im)))
        return complex(re.value, im.value)

    def set_phase(self, re: float, im: float):
        capi.check(self._fn("set_phase")(self._h, re, im))

    def advance(self, nsamples: int):
        capi.check(self._fn("advance")(self._h, int(nsamples)))

    def set_volk_gain(self, on: bool):
        capi.check(self._fn("set_volk_gain")(self._h, int(bool(on))))


class Xlator(_Op, _NcoMixin):
    _prefix = "qdsp_hip_xlate_cf32"

    def __init__(self, sample_rate: float = None, freq: float = None, phase_inc=None, device: int = 0,
                 max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        re, im = phase_inc if phase_inc is not None else phase_delta(sample_rate, freq)
        self.phase_inc = (re, im)
        capi.check(self._fn("create")(C.byref(self._h), device, re, im, max_block), self._prefix + "_create")


class Vfo(_Op, _HistMixin, _NcoMixin):
    """xlator(-offset) -> resampler in one kernel.  `taps`/interp/decim come from the caller
    (the window design stays on the host, SURVEY a5: qdsp_amd/host/dsp/window.h)."""

    _prefix = "qdsp_hip_xlate_fir_decim_cf32"

    def __init__(self, taps, interp: int, decim: int, phase_inc, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self._taps, p = _taps_ptr(taps)
        re, im = phase_inc
        capi.check(self._fn("create")(C.byref(self._h), device, p, len(self._taps), int(interp), int(decim), re, im,
                                      max_block), self._prefix + "_create")

    def configure(self, taps, interp: int, decim: int):
        self._taps, p = _taps_ptr(taps)
        capi.check(self._fn("configure")(self._h, p, len(self._taps), int(interp), int(decim)))

    def _out_size(self, n: int) -> int:
        return int(capi.check(self._fn("out_size")(self._h, n)))


class Channelizer:
    """Splitter -> N x VFO (src/dsp/routing.h:47-57, src/dsp/vfo.h) as one operator:
    qdsp_hip_chan_cf32_*.  process() returns an (nchan, outCount) array / tensor."""

    AUTO, DIRECT, FFT = 0, 1, 2

    def __init__(self, taps, interp: int, decim: int, phase_incs, device: int = 0, max_block: int = 1_000_000):
        self._L = capi.load()
        self._h = C.c_void_p()
        self.device = device
        self._taps, p = _taps_ptr(taps)
        incs = np.asarray(phase_incs, dtype=np.float32).reshape(-1, 2)
        self.nchan = len(incs)
        re, im = np.ascontiguousarray(incs[:, 0]), np.ascontiguousarray(incs[:, 1])
        fp = C.POINTER(C.c_float)
        capi.check(self._L.qdsp_hip_chan_cf32_create(C.byref(self._h), device, p, len(self._taps), int(interp), int(decim),
                                                     self.nchan, re.ctypes.data_as(fp), im.ctypes.data_as(fp), max_block),
                   "qdsp_hip_chan_cf32_create")

    def close(self):
        if self._h:
            self._L.qdsp_hip_chan_cf32_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_mode(self, mode: int):
        capi.check(self._L.qdsp_hip_chan_cf32_set_mode(self._h, int(mode)))

    def set_volk_gain(self, on: bool):
        capi.check(self._L.qdsp_hip_chan_cf32_set_volk_gain(self._h, int(bool(on))))

    def reset(self):
        capi.check(self._L.qdsp_hip_chan_cf32_reset(self._h))

    def out_size(self, n: int) -> int:
        return int(capi.check(self._L.qdsp_hip_chan_cf32_out_size(self._h, n)))

    _prefix = "qdsp_hip_chan_cf32"

    @property
    def history_len(self) -> int:
        return int(capi.check(self._L.qdsp_hip_chan_cf32_history_len(self._h)))

    def set_history_dev(self, hist):
        """The history_len raw input samples preceding the next call (device tensor)."""
        import torch

        assert hist.is_cuda and hist.is_contiguous() and hist.dtype == torch.complex64 and hist.numel() == self.history_len
        stream = torch.cuda.current_stream(hist.device).cuda_stream
        capi.check(self._L.qdsp_hip_chan_cf32_set_history_dev(self._h, hist.data_ptr(), stream))

    def set_history_ptr(self, ptr: int, stream: int):
        """The same from a raw device pointer (the receive buffer of the C ring, qdsp_hip_ring_complete) on HIP stream `stream`."""
        capi.check(self._L.qdsp_hip_chan_cf32_set_history_dev(self._h, int(ptr), int(stream)))

    def advance(self, n: int):
        capi.check(self._L.qdsp_hip_chan_cf32_advance(self._h, int(n)))

    def last_kernel(self):
        name = C.create_string_buffer(128)
        g, b, l = C.c_int(), C.c_int(), C.c_int()
        capi.check(self._L.qdsp_hip_last_kernel(self._h, name, 128, C.byref(g), C.byref(b), C.byref(l)))
        return {"name": name.value.decode(), "grid": g.value, "block": b.value, "lds_bytes": l.value}

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per process_dev over `iters` calls (torch events on the current stream)."""
        import torch

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            self.process(x, out)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def process(self, x, out=None):
        if _is_torch(x):
            import torch

            assert x.is_cuda and x.is_contiguous() and x.dtype == torch.complex64
            n, no = x.numel(), self.out_size(x.numel())
            if out is None:
                out = torch.empty((self.nchan, max(no, 1)), dtype=torch.complex64, device=x.device)
            assert out.is_contiguous() and out.shape[0] == self.nchan and out.shape[1] >= no
            stream = torch.cuda.current_stream(x.device).cuda_stream
            rc = self._L.qdsp_hip_chan_cf32_process_dev(self._h, x.data_ptr(), n, out.data_ptr(), out.shape[1], stream)
            capi.check(int(rc), "qdsp_hip_chan_cf32_process_dev")
            return out[:, :no]
        a = np.ascontiguousarray(x, dtype=np.complex64)
        no = self.out_size(a.size)
        y = np.empty((self.nchan, max(no, 1)), dtype=np.complex64)
        rc = self._L.qdsp_hip_chan_cf32_process(self._h, a.ctypes.data, a.size, y.ctypes.data, y.shape[1])
        capi.check(rc, "qdsp_hip_chan_cf32_process")
        return y[:, :no]


def synth_iq(count: int, first_sample: int = 0, seed: int = 1234, device: int = 0, out=None):
    """Counter-based uniform IQ generated on the device (measurement input)."""
    import torch

    if out is None:
        out = torch.empty(count, dtype=torch.complex64, device=f"cuda:{device}")
    stream = torch.cuda.current_stream(out.device).cuda_stream
    capi.check(capi.load().qdsp_hip_synth_iq_dev(device, out.data_ptr(), first_sample, count, seed, stream),
               "qdsp_hip_synth_iq_dev")
    return out


def device_info(device: int = 0) -> dict:
    L = capi.load()
    name, arch, cus = C.create_string_buffer(256), C.create_string_buffer(256), C.c_int()
    capi.check(L.qdsp_hip_device_info(device, name, 256, arch, 256, C.byref(cus)))
    return {"name": name.value.decode(), "arch": arch.value.decode(), "compute_units": cus.value}


__all__ = ["Fir", "Resampler", "Xlator", "Vfo", "Channelizer", "synth_iq", "phase_delta", "device_info"]


class Math:
    """Add / Substract / Multiply of two streams (src/dsp/math.h:7-145): qdsp_hip_math_*."""

    ADD, SUB, MUL = 0, 1, 2

    def __init__(self, op: int, complex_data: bool = True, device: int = 0, max_block: int = 1_000_000):
        self._L = capi.load()
        self._h = C.c_void_p()
        self.complex_data = complex_data
        capi.check(self._L.qdsp_hip_math_create(C.byref(self._h), device, int(op), int(complex_data), max_block), "qdsp_hip_math_create")

    def close(self):
        if self._h:
            self._L.qdsp_hip_math_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def process(self, a, b, out=None):
        if _is_torch(a):
            import torch

            dt = torch.complex64 if self.complex_data else torch.float32
            assert a.is_cuda and b.is_cuda and a.dtype == dt and b.dtype == dt and a.numel() == b.numel()
            assert a.is_contiguous() and b.is_contiguous()
            if out is None:
                out = torch.empty_like(a)
            stream = torch.cuda.current_stream(a.device).cuda_stream
            capi.check(self._L.qdsp_hip_math_process_dev(self._h, a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), stream),
                       "qdsp_hip_math_process_dev")
            return out
        dt = np.complex64 if self.complex_data else np.float32
        x, y = np.ascontiguousarray(a, dtype=dt), np.ascontiguousarray(b, dtype=dt)
        assert x.size == y.size
        o = np.empty_like(x)
        capi.check(self._L.qdsp_hip_math_process(self._h, x.ctypes.data, y.ctypes.data, x.size, o.ctypes.data), "qdsp_hip_math_process")
        return o



def _per_chan(v, nchan: int) -> np.ndarray:
    """A scalar, or one value per channel, as `nchan` floats."""
    return np.broadcast_to(np.asarray(v, dtype=np.float32), (nchan,))


_REAL_COMPLEX = (("real", "float32"), ("complex", "complex64"))


def _parse_kind(k, kinds, what: str, exact: bool = False) -> int:
    """The kind a `kind_or_dtype` argument spells: its index in `kinds`, one (word, dtype name) per kind.  By default any int passes
    through for the library to judge, and a numpy or torch dtype or scalar type is known by the dtype name in the last dotted part
    of its str.  `exact` (Deframer): the index, the word, or the dtype's name, bare or as torch prints it, and nothing else."""
    if exact:
        name = k if isinstance(k, (int, str)) else getattr(k, "__name__", str(k))
    elif isinstance(k, (int, np.integer)) and not isinstance(k, bool):
        return int(k)
    else:
        name = str(k).rsplit(".", 1)[-1]
    for kind, (word, dt) in enumerate(kinds):
        if (name in (kind, word, dt, "torch." + dt)) if exact else ((isinstance(k, str) and k == word) or dt in name):
            return kind
    raise ValueError(f"{what}: {' or '.join(dt for _, dt in kinds)} rows, not {k!r}")


def _row_type(kind: int):
    """The numpy sample type of a REAL / COMPLEX kind's rows."""
    return np.complex64 if kind == 1 else np.float32


def _tail(width: int) -> tuple:
    """The trailing shape of samples `width` elements wide: stereo_t pairs sit in a last dimension of 2."""
    return (2,) if width == 2 else ()


def _in_counts_ptr(in_counts, nchan, device):
    """The device pointer of an optional int32 tensor of per-row input counts (None: every row has the call's count)."""
    import torch

    if in_counts is None:
        return None
    assert in_counts.is_cuda and in_counts.dtype == torch.int32 and in_counts.is_contiguous() and in_counts.numel() == nchan
    assert in_counts.device == device
    return in_counts.data_ptr()


class _Rows(_Op):
    """An operator over `nchan` channel rows and its three entry forms.  numpy input: the host entry point (one channel); a tensor of
    one row: *_process_dev on torch's current stream; a tensor of `nchan` rows: `process_batch`.  A class states what is its own:

        _np, _out_np      the numpy type of an input / output sample; the torch dtype has the same name (_out_np None: as the input)
        _iw, _ow          2 where a sample is a stereo_t pair, a trailing dimension of 2; else 1.  Also the unit of the row stride.
        _emits            the outputs of a call of n samples: "n"; "returned" (_OutSize): at most out_size(n), the call returns the
                          count; "counts" (_Counts): out_size(n) slots per row and a count per row
        _per              the elements of one output (a Deframer's frame: frame_bytes)
        _takes_in_counts  the batch entry point takes an int32 tensor of per-row input counts
        _flat             the 1-D form reads `nchan` rows back to back (the demodulators); every other class refuses nchan > 1 there
        _batch_fn         the batch entry point's name, where it is not <prefix>_process_batch_dev"""

    _np, _out_np = np.float32, None
    _iw = _ow = 1
    _emits = "n"
    _per = 1
    _takes_in_counts = False
    _flat = False
    _batch_fn = None

    def _torch_types(self):
        import torch

        return torch, getattr(torch, np.dtype(self._np).name), getattr(torch, np.dtype(self._out_np or self._np).name)

    def _slots(self, n: int) -> int:
        """The elements an output row needs for a call of `n` samples."""
        return (n if self._emits == "n" else self.out_size(n)) * self._per

    def _result(self, y):
        """The 1-D result as the class shows it (Deframer: frames by bytes)."""
        return y

    def process(self, x, out=None):
        if _is_torch(x):
            return self.process_batch(x, out) if x.dim() == 1 + self._iw else self._process_dev(x, out)
        a = np.ascontiguousarray(x, dtype=self._np)
        assert self._flat or (a.ndim == self._iw and a.shape[1:] == _tail(self._iw)), a.shape
        n = a.size // self._iw
        y = np.empty((max(self._slots(n), 1),) + _tail(self._ow), dtype=self._out_np or self._np)
        rc = capi.check(self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data), self._prefix + "_process")
        return self._result(y[:(n if self._emits == "n" else rc) * self._per])

    def _process_dev(self, x, out=None):
        torch, idt, odt = self._torch_types()
        assert x.is_cuda and x.is_contiguous() and x.dtype == idt, "one contiguous row"
        assert self._flat or (self.nchan == 1 and x.dim() == self._iw and tuple(x.shape[1:]) == _tail(self._iw)), "one contiguous row"
        n = x.numel() // self._iw // self.nchan
        assert n * self._iw * self.nchan == x.numel(), "whole rows"
        assert out is None or (out.is_cuda and out.is_contiguous() and out.dtype == odt and out.dim() == self._ow and tuple(out.shape[1:]) == _tail(self._ow))
        cap = self._slots(n) * self.nchan
        if out is None:
            out = torch.empty((max(cap, 1),) + _tail(self._ow), dtype=odt, device=x.device)
        assert out.shape[0] >= cap
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = capi.check(int(self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)), self._prefix + "_process_dev")
        if self._emits == "n":
            no = n * self.nchan
        else:
            no = rc if self._emits == "returned" else int(self.counts()[0])
        return self._result(out[:no * self._per])

    def process_batch(self, x, out=None, count: int = None):
        """Channel c = row c of the tensor `x`, (nchan, n) or, of stereo_t samples, (nchan, n, 2).  Rows may be padded (x.stride(0)
        beyond the row: another operator's batch output, or a slice of it) and `count` may stop short of them.  Returns the
        (nchan, outputs) view of `out`, or of new rows.  out=x works in place unless the class says that they may not overlap."""
        return self._batch(x, out, count)

    def _batch(self, x, out, count, in_counts=None, counts=None):
        torch, idt, odt = self._torch_types()
        iw, ow = self._iw, self._ow
        assert x.is_cuda and x.dtype == idt and x.dim() == 1 + iw and x.shape[0] == self.nchan and x.stride(1) == iw and x.stride(0) % iw == 0
        assert iw == 1 or (x.shape[2] == 2 and x.stride(2) == 1)
        n = x.shape[1] if count is None else int(count)
        cap = self._slots(n)
        if out is None:
            out = torch.empty((self.nchan, max(cap, 1)) + _tail(ow), dtype=odt, device=x.device)
        assert out.is_cuda and out.dtype == odt and out.dim() == 1 + ow and out.shape[0] == self.nchan and out.shape[1] >= cap
        assert out.stride(1) == ow and out.stride(0) % ow == 0 and (ow == 1 or (out.shape[2] == 2 and out.stride(2) == 1))
        mid = (_in_counts_ptr(in_counts, self.nchan, x.device),) if self._takes_in_counts else ()
        last = ()
        if self._emits == "counts":
            if counts is None:
                counts = torch.empty(self.nchan, dtype=torch.int32, device=x.device)
            assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == self.nchan
            last = (counts.data_ptr(),)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        name = self._batch_fn or self._prefix + "_process_batch_dev"
        rc = getattr(self._L, name)(self._h, x.data_ptr(), n, x.stride(0) // iw, *mid, out.data_ptr(), out.stride(0) // ow, *last, stream)
        rc = capi.check(int(rc), name)
        if self._emits == "counts":
            return out[:, :cap], counts
        return out[:, :n if self._emits == "n" else rc]

    def process_ex(self, x, in_link: int, count: int, out, out_link: int):
        """The block-graph entry point on raw pointers (host or device, QDSP_HIP_LINK_* codes)."""
        return capi.check(self._fn("process_ex")(self._h, int(x), int(in_link), int(count), int(out), int(out_link)))

    def set_done_event(self, ev: int):
        capi.check(self._L.qdsp_hip_set_done_event(self._h, C.c_void_p(ev)))

    def _time_count(self, x) -> int:
        return x.numel() // self.nchan

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per launch of `iters` back-to-back process_dev calls over the nchan rows of `x`, back to back
        (qdsp_hip_time_process_dev)."""
        import torch

        stream = torch.cuda.current_stream(x.device).cuda_stream
        ms = C.c_float()
        rc = self._L.qdsp_hip_time_process_dev(self._h, x.data_ptr(), self._time_count(x), out.data_ptr(), stream, iters, C.byref(ms))
        capi.check(rc, "qdsp_hip_time_process_dev")
        return float(ms.value)


class _OutSize:
    """For a class whose calls emit at most `out_size(n)` outputs per row and return the count."""

    _emits = "returned"

    def out_size(self, n: int) -> int:
        """The most outputs per row a call of `n` samples per row can emit: the slots an output row needs.  FeedForwardAgc: what
        the next call would emit."""
        return int(capi.check(int(self._fn("out_size")(self._h, int(n))), self._prefix + "_out_size"))


class _Counts(_OutSize):
    """... and whose rows each emit a count of their own."""

    _emits = "counts"

    def counts(self) -> np.ndarray:
        """The outputs per row of the last call (synchronises the device)."""
        c = np.zeros(self.nchan, dtype=np.int32)
        capi.check(self._fn("get_counts")(self._h, c.ctypes.data_as(C.POINTER(C.c_int))))
        return c


class _Demod(_Rows):
    """Complex in, real out: one float per sample, or a stereo_t {l, r} pair (`_ow` 2).  The 1-D form of a handle of `nchan`
    channels reads their rows back to back."""

    nchan = 1
    _np, _out_np = np.complex64, np.float32
    _flat = True


class FmDemod(_Demod):
    """FloatFMDemod (stereo=False, float out) / FMDemod (stereo=True, {l, r} with l == r) of src/dsp/demodulator.h:33-187,
    bit-identical to the reference loop; `nchan` channels per launch, each with its own deviation and carried phase."""

    _prefix = "qdsp_hip_demod"

    def __init__(self, sample_rate, deviation, stereo: bool = False, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self._ow = 2 if stereo else 1
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, 1 if stereo else 0, self.nchan, max_block), "qdsp_hip_demod_create")
        rates, devs = _per_chan(sample_rate, self.nchan), _per_chan(deviation, self.nchan)
        for c in range(self.nchan):
            self.set_fm(float(rates[c]), float(devs[c]), c)

    def set_fm(self, sample_rate: float, deviation: float, chan: int = -1):
        capi.check(self._fn("set_fm")(self._h, int(chan), sample_rate, deviation), "qdsp_hip_demod_set_fm")

    def get_phase(self, chan: int = 0) -> float:
        v = C.c_float()
        capi.check(self._fn("get_phase")(self._h, int(chan), C.byref(v)))
        return np.float32(v.value)

    def set_phase(self, phase: float, chan: int = -1):
        capi.check(self._fn("set_phase")(self._h, int(chan), phase))

    def reset(self):
        capi.check(self._fn("reset")(self._h))


class AmDemod(_Demod):
    """AMDemod (src/dsp/demodulator.h:332-378): |x| minus the mean of the call's |x|, per channel."""

    _prefix = "qdsp_hip_demod"

    def __init__(self, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, 2, self.nchan, max_block), "qdsp_hip_demod_create")


def ssb_phase_delta(sample_rate: float, bandwidth: float, mode: int):
    """phaseDelta exactly as SSBDemod::init computes it (demodulator.h:408-419): float operands, the float cos/sin."""
    theta = np.float32(np.float32(bandwidth) / np.float32(sample_rate)) * FL_M_PI
    if mode == SsbDemod.DSB:
        return 1.0, 0.0
    if mode == SsbDemod.LSB:
        theta = np.float32(-np.float32(np.float32(bandwidth) / np.float32(sample_rate))) * FL_M_PI
    elif mode != SsbDemod.USB:
        raise ValueError(f"mode {mode}")
    return float(_libm().cosf(C.c_float(theta))), float(_libm().sinf(C.c_float(theta)))


class SsbDemod(_Demod, _NcoMixin):
    """SSBDemod (src/dsp/demodulator.h:380-497): the xlator's NCO, real part out."""

    USB, LSB, DSB = 0, 1, 2
    _prefix = "qdsp_hip_ssb_cf32"
    _batch_fn = "qdsp_hip_demod_process_batch_dev"     # (no batch entry point of its own: the demodulators' refuses the handle)

    def __init__(self, sample_rate: float = None, bandwidth: float = None, mode: int = 0, phase_inc=None, device: int = 0,
                 max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        re, im = phase_inc if phase_inc is not None else ssb_phase_delta(sample_rate, bandwidth, mode)
        self.phase_inc = (re, im)
        capi.check(self._fn("create")(C.byref(self._h), device, re, im, max_block), "qdsp_hip_ssb_cf32_create")


__all__ += ["FmDemod", "AmDemod", "SsbDemod", "ssb_phase_delta"]


class Deemp(_Rows):
    """BFMDeemp (src/dsp/filter.h:90-173): y[i] = alpha x[i] + (1 - alpha) y[i-1], alpha = dt / (tau + dt) in float, run as
    an FP64 prefix scan (include/qdsp_hip.h).  stereo=True: stereo_t rows, shape (n, 2), l and r filtered independently;
    stereo=False: float rows.  `nchan` channels per launch, each with its own alpha and state.  numpy input: the host entry
    point (one channel); a 1-D / (n, 2) torch tensor: *_process_dev; (nchan, n) / (nchan, n, 2): `process_batch`, where out=x
    filters in place."""

    _prefix = "qdsp_hip_deemp"

    def __init__(self, sample_rate, tau, stereo: bool = True, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self._stereo = bool(stereo)
        self._iw = self._ow = 2 if stereo else 1
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, 1 if stereo else 0, self.nchan, max_block), "qdsp_hip_deemp_create")
        rates, taus = _per_chan(sample_rate, self.nchan), _per_chan(tau, self.nchan)
        for c in range(self.nchan):
            self.set(float(rates[c]), float(taus[c]), c)

    def set(self, sample_rate: float, tau: float, chan: int = -1):
        capi.check(self._fn("set")(self._h, int(chan), sample_rate, tau), "qdsp_hip_deemp_set")

    def bypass(self, on: bool):
        capi.check(self._fn("set_bypass")(self._h, int(bool(on))))

    def alpha(self, chan: int = 0):
        v = C.c_float()
        capi.check(self._fn("get_alpha")(self._h, int(chan), C.byref(v)))
        return np.float32(v.value)

    def get_state(self, chan: int = 0):
        """The carried output, rounded to float: (l, r), or one value (mono)."""
        l, r = C.c_float(), C.c_float()
        capi.check(self._fn("get_state")(self._h, int(chan), C.byref(l), C.byref(r)))
        return (np.float32(l.value), np.float32(r.value)) if self._stereo else np.float32(l.value)

    def set_state(self, l: float, r: float = 0.0, chan: int = -1):
        capi.check(self._fn("set_state")(self._h, int(chan), l, r))

    def reset(self):
        capi.check(self._fn("reset")(self._h))

    def _time_count(self, x) -> int:
        return x.shape[0] // self.nchan


__all__ += ["Deemp"]


class _RowOp(_Rows):
    """A row operator whose handle has a reset.  (The demodulators and Deemp name their own: not every one of them has one.)"""

    nchan = 1

    def reset(self):
        capi.check(self._fn("reset")(self._h))


class Squelch(_RowOp):
    """dsp::Squelch (src/dsp/processing.h:424-489): a call whose mean |x| is at least `level` dB is copied, any other is
    zeroed; `nchan` channels per launch, each with its own level (a scalar or one value per channel)."""

    _prefix = "qdsp_hip_squelch"
    _np = np.complex64

    def __init__(self, level=-50.0, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, max_block), "qdsp_hip_squelch_create")
        levels = _per_chan(level, self.nchan)
        for c in range(self.nchan):
            self.set_level(float(levels[c]), c)

    def set_level(self, level: float, chan: int = -1):
        capi.check(self._fn("set_level")(self._h, int(chan), level), "qdsp_hip_squelch_set_level")

    def is_open(self, chan: int = 0) -> bool:
        """The decision of the last call (synchronises the device)."""
        v = C.c_int()
        capi.check(self._fn("get_open")(self._h, int(chan), C.byref(v)))
        return bool(v.value)


class Agc(_RowOp):
    """dsp::AGC (src/dsp/processing.h:83-145): the call scaled by 1 / level; level decays by fall_rate / sample_rate dB per
    sample and follows the call's maximum.  `nchan` channels per launch, each with its own rates and level."""

    _prefix = "qdsp_hip_agc"

    def __init__(self, fall_rate, sample_rate, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, max_block), "qdsp_hip_agc_create")
        falls, rates = _per_chan(fall_rate, self.nchan), _per_chan(sample_rate, self.nchan)
        for c in range(self.nchan):
            self.set(float(falls[c]), float(rates[c]), c)

    def set(self, fall_rate: float, sample_rate: float, chan: int = -1):
        capi.check(self._fn("set")(self._h, int(chan), fall_rate, sample_rate), "qdsp_hip_agc_set")

    def level(self, chan: int = 0):
        """The carried level (synchronises the device)."""
        v = C.c_float()
        capi.check(self._fn("get_level")(self._h, int(chan), C.byref(v)))
        return np.float32(v.value)

    def set_level(self, level: float, chan: int = -1):
        capi.check(self._fn("set_level")(self._h, int(chan), level))


__all__ += ["Squelch", "Agc"]


def stereo_pilot_taps(sample_rate: float) -> np.ndarray:
    """StereoFMDemod's pilot filter (src/dsp/demodulator.h:217): BlackmanBandpassWindow(1000, 1000, 19000, sampleRate) with the
    reference's tap count, every step in float in the reference's order (src/dsp/window.h:105-140) with glibc's sinf / cosf, as
    the C++ mirror's dsp/window.h computes it (tests/test_stereo_fm_cpu.py pins both to the CPU oracle bit for bit)."""
    f32, m = np.float32, _libm()
    sinf = lambda v: f32(m.sinf(C.c_float(v)))    # noqa: E731
    cosf = lambda v: f32(m.cosf(C.c_float(v)))    # noqa: E731
    fs, cutoff, trans, offset = f32(sample_rate), f32(1000.0), f32(1000.0), f32(19000.0)
    n = int(f32(4.0) / f32(trans / fs))
    n = max(n, 4)
    n += 1 if n % 2 == 0 else 0
    fc = min(f32(cutoff / fs), f32(1.0))
    tc = f32(n)
    window = f32(f32(f32(0.42) - f32(f32(0.5) * cosf(f32(f32(f32(2.0) * FL_M_PI) / tc)))) + f32(f32(0.8) * cosf(f32(f32(f32(4.0) * FL_M_PI) / tc))))
    taps, total = np.zeros(n, f32), f32(0.0)
    for i in range(n):
        d = f32(f32(i) - f32(tc / f32(2.0)))
        with np.errstate(all="ignore"):
            v = f32(f32(sinf(f32(f32(f32(f32(2.0) * FL_M_PI) * fc) * d)) / d) * window)
        taps[i] = v
        total = f32(total + v)
    shift = f32(f32(f32(2.0) * f32(offset / fs)) * FL_M_PI)
    for i in range(n):
        taps[i] = f32(f32(taps[i] * cosf(f32(shift * f32(i)))) * f32(1.0)) / total
    return taps


class StereoFmDemod(_Demod):
    """dsp::StereoFMDemod (src/dsp/demodulator.h:189-330): FloatFMDemod, the 19 kHz pilot FIR, AGC(20, sampleRate) and the
    matrix {m + m p^2, m - m p^2}; `nchan` channels per call, each with its own deviation, phase, filter history and level.
    `pilot_taps` (shared by all channels) default to the reference's for `sample_rate` (a scalar then)."""

    _prefix = "qdsp_hip_stereo_fm"
    _ow = 2

    def __init__(self, sample_rate, deviation, nchan: int = 1, pilot_taps=None, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        self._count = 0
        rates, devs = _per_chan(sample_rate, self.nchan), _per_chan(deviation, self.nchan)
        if pilot_taps is None:
            assert np.all(rates == rates[0]), "one pilot filter for all channels: pass pilot_taps"
            pilot_taps = stereo_pilot_taps(float(rates[0]))
        t, tp = _taps_ptr(pilot_taps)
        self.ntaps = int(t.size)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, tp, self.ntaps, max_block), "qdsp_hip_stereo_fm_create")
        for c in range(self.nchan):
            self.set_fm(float(rates[c]), float(devs[c]), c)

    def process(self, x, out=None):
        y = super().process(x, out)
        if not _is_torch(x):
            self._count = len(y)
        return y

    def _process_dev(self, x, out=None):
        y = super()._process_dev(x, out)
        self._count = x.numel() // self.nchan
        return y

    def process_batch(self, x, out=None, count: int = None):
        """Channel c = row c of the 2-D complex64 tensor `x` (rows may be padded); returns (nchan, count, 2) float32."""
        y = super().process_batch(x, out, count)
        self._count = y.shape[1]
        return y

    def process_ex(self, x, in_link: int, count: int, out, out_link: int):
        rc = super().process_ex(x, in_link, count, out, out_link)
        self._count = int(count)
        return rc

    def set_fm(self, sample_rate: float, deviation: float, chan: int = -1):
        capi.check(self._fn("set_fm")(self._h, int(chan), sample_rate, deviation), "qdsp_hip_stereo_fm_set_fm")

    def set_pilot_taps(self, taps):
        """New taps for all channels; the filter history is zeroed, phase and level stay."""
        t, tp = _taps_ptr(taps)
        capi.check(self._fn("set_pilot_taps")(self._h, tp, int(t.size)), "qdsp_hip_stereo_fm_set_pilot_taps")
        self.ntaps = int(t.size)

    def get_phase(self, chan: int = 0):
        v = C.c_float()
        capi.check(self._fn("get_phase")(self._h, int(chan), C.byref(v)))
        return np.float32(v.value)

    def set_phase(self, phase: float, chan: int = -1):
        capi.check(self._fn("set_phase")(self._h, int(chan), phase))

    def level(self, chan: int = 0):
        """The carried AGC level (synchronises the device)."""
        v = C.c_float()
        capi.check(self._fn("get_level")(self._h, int(chan), C.byref(v)))
        return np.float32(v.value)

    def set_level(self, level: float, chan: int = -1):
        capi.check(self._fn("set_level")(self._h, int(chan), level))

    def pilot_ptr(self):
        """(device pointer, row stride in floats) of the library's own rows of the last call's filtered pilot f; the next
        call overwrites them (qdsp_hip_stereo_fm_pilot_dev)."""
        p, stride = C.c_void_p(), C.c_int64()
        capi.check(self._fn("pilot_dev")(self._h, C.byref(p), C.byref(stride)), "qdsp_hip_stereo_fm_pilot_dev")
        return p.value or 0, int(stride.value)

    def pilot(self):
        """The last call's filtered pilot f as a new (nchan, count) float32 tensor (synchronises the device)."""
        import torch

        p, stride = self.pilot_ptr()
        rows = torch.empty((self.nchan, max(stride, 1)), dtype=torch.float32, device=f"cuda:{self.device}")
        if p and self._count:
            torch.cuda.synchronize(self.device)
            capi.check(self._L.qdsp_hip_memcpy_d2d(self.device, rows.data_ptr(), p, self.nchan * stride * 4), "qdsp_hip_memcpy_d2d")
        return rows[:, :self._count if p else 0]

    def reset(self):
        capi.check(self._fn("reset")(self._h))
        self._count = 0

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per call of `iters` back-to-back process_dev calls over the nchan rows of `x` (qdsp_hip_time_process_dev)."""
        ms = super().time_dev(x, out, iters)
        self._count = x.numel() // self.nchan
        return ms


__all__ += ["StereoFmDemod", "stereo_pilot_taps"]


class FeedForwardAgc(_OutSize, _RowOp):
    """dsp::FeedForwardAGC<T> (src/dsp/processing.h:147-233): every sample divided by the peak of the `window` samples from it on
    (a sliding-window maximum, floor 1e-4).  `kind_or_dtype`: 0 / "real" / float32 for float rows, 1 / "complex" / complex64 for
    complex_t rows (the level follows |re| alone, as the reference's fastAmplitude does).  The output lags the input by
    window - 1 samples: a call of n samples returns `out_size(n)` outputs, none at all while the history fills.  `nchan` rows per
    launch share one fill.  `out` may not overlap the input."""

    _prefix = "qdsp_hip_ffagc"
    REAL, COMPLEX = 0, 1

    def __init__(self, kind_or_dtype=1, nchan: int = 1, device: int = 0, max_block: int = 1_000_000, window: int = 1024):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        self.kind = _parse_kind(kind_or_dtype, _REAL_COMPLEX, "FeedForwardAgc")
        self._np = _row_type(self.kind)
        self.window = int(window)
        capi.check(self._fn("create")(C.byref(self._h), device, self.kind, self.nchan, max_block, self.window), "qdsp_hip_ffagc_create")

    @classmethod
    def _kind_of(cls, k) -> int:
        return _parse_kind(k, _REAL_COMPLEX, cls.__name__)

    def fill(self) -> int:
        """The samples taken in and not yet output (per row)."""
        return capi.check(self._fn("fill")(self._h), "qdsp_hip_ffagc_fill")

    def get_history(self, chan: int = 0) -> np.ndarray:
        h = np.zeros(max(self.window - 1, 1), dtype=self._np)
        capi.check(self._fn("get_history")(self._h, int(chan), h.ctypes.data), "qdsp_hip_ffagc_get_history")
        return h[:self.fill()]

    def set_history(self, hist, chan: int = -1):
        h = np.ascontiguousarray(hist, dtype=self._np)
        capi.check(self._fn("set_history")(self._h, int(chan), h.ctypes.data, h.size), "qdsp_hip_ffagc_set_history")


__all__ += ["FeedForwardAgc"]


class ComplexAgc(_RowOp):
    """dsp::ComplexAGC (src/dsp/processing.h:235-298): out[i] = x[i] g; g += (set_point - |out[i]|) rate; g = min(g, max_gain),
    per sample, run as an FP64 clamped prefix scan (include/qdsp_hip.h: complex AGC).  `nchan` complex64 rows per launch, each
    with its own parameters (scalars or one value per channel) and gain.  A row the scan does not cover in a call -- a NaN or Inf
    sample, rate |x| > 1, a negative, NaN or Inf gain, set_point rate < 0 -- is run by the reference's float loop on the device
    instead, serially.  Entry points by input as for Squelch and Agc; out=x works in place."""

    _prefix = "qdsp_hip_cagc"
    _np = np.complex64

    def __init__(self, set_point=1.0, max_gain=1e5, rate=1e-3, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, max_block), "qdsp_hip_cagc_create")
        sps, mgs, rts = _per_chan(set_point, self.nchan), _per_chan(max_gain, self.nchan), _per_chan(rate, self.nchan)
        for c in range(self.nchan):
            self.set(float(sps[c]), float(mgs[c]), float(rts[c]), c)

    def set(self, set_point: float, max_gain: float, rate: float, chan: int = -1):
        """Takes effect from the next call."""
        capi.check(self._fn("set")(self._h, int(chan), set_point, max_gain, rate), "qdsp_hip_cagc_set")

    def get_gain(self, chan: int = 0) -> float:
        """The carried gain, FP64 (synchronises the device)."""
        v = C.c_double()
        capi.check(self._fn("get_gain")(self._h, int(chan), C.byref(v)))
        return float(v.value)

    def set_gain(self, gain: float, chan: int = -1):
        capi.check(self._fn("set_gain")(self._h, int(chan), float(gain)))


__all__ += ["ComplexAgc"]


class CostasLoop(_RowOp):
    """dsp::CostasLoop<ORDER> (src/dsp/pll.h:47-102), ORDER 2, 4 or 8: out = vco x; the order's phase error of out, clamped, moves
    the frequency (beta) and the phase (alpha); vco = exp(-j phase).  One row per lane, 16 rows to a wave (include/qdsp_hip.h: Costas
    loop).  `nchan` complex64 rows per launch, each with its own loop bandwidth (a scalar or one value per channel), frequency and
    phase (FP64, on the device).  Entry points by input as for Squelch and Agc; out=x works in place."""

    _prefix = "qdsp_hip_costas"
    _np = np.complex64

    def __init__(self, order: int, bandwidth, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.order = int(order)
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, self.order, self.nchan, max_block), "qdsp_hip_costas_create")
        bws = _per_chan(bandwidth, self.nchan)
        if np.all(bws == bws[0]):
            self.set_bandwidth(float(bws[0]))
        else:
            for c in range(self.nchan):
                self.set_bandwidth(float(bws[c]), c)

    def set_bandwidth(self, bandwidth: float, chan: int = -1):
        """Takes effect from the next call; finite and >= 0."""
        capi.check(self._fn("set_bandwidth")(self._h, int(chan), bandwidth), "qdsp_hip_costas_set_bandwidth")

    def gains(self, chan: int = 0):
        """(alpha, beta) in use, the reference's floats."""
        a, b = C.c_float(), C.c_float()
        capi.check(self._fn("get_gains")(self._h, int(chan), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def get_state(self, chan: int = 0):
        """The carried (frequency, phase), FP64 (synchronises the device)."""
        f, p = C.c_double(), C.c_double()
        capi.check(self._fn("get_state")(self._h, int(chan), C.byref(f), C.byref(p)))
        return float(f.value), float(p.value)

    def set_state(self, freq: float, phase: float, chan: int = -1):
        capi.check(self._fn("set_state")(self._h, int(chan), float(freq), float(phase)), "qdsp_hip_costas_set_state")


__all__ += ["CostasLoop"]


class MmClockRecovery(_Counts, _RowOp):
    """dsp::MMClockRecovery<T> (src/dsp/clock_recovery.h:68-243): Mueller & Mueller symbol timing.  Every symbol is the 8-tap MMSE
    interpolation of the input at the loop's position (129 fractional steps, the table in `interp_taps()`), and the type's phase
    error of the symbol moves the symbol period (`gain_omega`, within omega (1 +- rel_limit)) and the position (`mu_gain`).
    `kind_or_dtype`: 0 / "real" / float32 for float rows (MSKDemod), 1 / "complex" / complex64 for complex_t rows (PSKDemod).
    One row per lane, 16 rows to a wave (include/qdsp_hip.h: symbol timing); `nchan` rows per launch, each with its own parameters
    (scalars or one value per channel) and state.  A call of n samples emits a data-dependent number of symbols per row, at most
    `out_size(n)`: `process` returns them (one row), `process_batch` the padded rows and the counts."""

    _prefix = "qdsp_hip_mmcr"
    REAL, COMPLEX = 0, 1

    def __init__(self, kind_or_dtype, omega, gain_omega=0.01 * 0.01 / 4, mu_gain=0.01, rel_limit=0.005, nchan: int = 1,
                 device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        self.kind = _parse_kind(kind_or_dtype, _REAL_COMPLEX, "MmClockRecovery")
        self._np = _row_type(self.kind)
        par = [_per_chan(v, self.nchan) for v in (omega, gain_omega, mu_gain, rel_limit)]
        capi.check(self._fn("create")(C.byref(self._h), device, self.kind, self.nchan, max_block, *(float(v[0]) for v in par)),
                   "qdsp_hip_mmcr_create")
        if any(np.any(v != v[0]) for v in par):
            self._set_rows(par)

    def _set_rows(self, par):
        """omega, gain_omega, mu_gain and rel_limit of every channel, in an order in which no step leaves the parameter rule."""
        for c in range(self.nchan):
            # (one at a time a change may leave the rule for a moment: gains and limit that fit every omega first)
            self.set_gains(0.0, 0.0, c)
            self.set_limit(0.0, c)
            self.set_omega(float(par[0][c]), c)
            self.set_limit(float(par[3][c]), c)
            self.set_gains(float(par[1][c]), float(par[2][c]), c)

    def set_omega(self, omega: float, chan: int = -1):
        """Samples per symbol; also restarts the loop's period there.  Takes effect from the next call."""
        capi.check(self._fn("set_omega")(self._h, int(chan), omega), "qdsp_hip_mmcr_set_omega")

    def set_gains(self, gain_omega: float, mu_gain: float, chan: int = -1):
        capi.check(self._fn("set_gains")(self._h, int(chan), gain_omega, mu_gain), "qdsp_hip_mmcr_set_gains")

    def set_limit(self, rel_limit: float, chan: int = -1):
        capi.check(self._fn("set_limit")(self._h, int(chan), rel_limit), "qdsp_hip_mmcr_set_limit")

    def get_state(self, chan: int = 0):
        """(mu, dynOmega, next): next = samples from the end of the input so far to the next symbol (synchronises the device)."""
        mu, dyn, nx = C.c_float(), C.c_float(), C.c_int()
        capi.check(self._fn("get_state")(self._h, int(chan), C.byref(mu), C.byref(dyn), C.byref(nx)))
        return float(mu.value), float(dyn.value), int(nx.value)

    def set_state(self, mu: float, dyn_omega: float, next: int, chan: int = -1):
        capi.check(self._fn("set_state")(self._h, int(chan), float(mu), float(dyn_omega), int(next)), "qdsp_hip_mmcr_set_state")

    def interp_taps(self) -> np.ndarray:
        t = np.zeros((129, 8), dtype=np.float32)
        capi.check(self._fn("get_interp_taps")(self._h, t.ctypes.data_as(C.POINTER(C.c_float))))
        return t

    def set_interp_taps(self, taps):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        assert t.shape == (129, 8), t.shape
        capi.check(self._fn("set_interp_taps")(self._h, t.ctypes.data_as(C.POINTER(C.c_float))), "qdsp_hip_mmcr_set_interp_taps")

    def process_batch(self, x, out=None, count: int = None, counts=None):
        """Channel c = row c of the 2-D tensor `x` (rows may be padded: x.stride(0) >= count).  Returns (rows, counts): the
        (nchan, out_size(count)) view of `out`, row c's symbols in its first counts[c] slots and the rest untouched, and the
        counts as an int32 device tensor (`counts`, or a new one).  Asynchronous; `out` may not overlap `x`."""
        return self._batch(x, out, count, counts=counts)


__all__ += ["MmClockRecovery"]


class RowFir(_RowOp):
    """dsp::FIR<T> (src/dsp/filter.h:51-74) over `nchan` channel rows in one launch (include/qdsp_hip.h: FIR over channel rows):
    y[c][i] = sum_k taps[c][k] x[c][i - (T - 1) + k], every output component the chain acc = fmaf(taps[k], x, acc) in tap order --
    the bits of `Fir(...).set_mode(Fir.DIRECT)` row by row.  `kind_or_dtype` as for MmClockRecovery (float32 or complex64 rows);
    `taps`: one row for all channels or an (nchan, T) array.  Entry points by input as for Squelch and Agc; `out` may not overlap
    the input.  TILE: the kernel's outputs per workgroup; TAP_GROUP: the taps per unrolled group of its tap loop."""

    _prefix = "qdsp_hip_rowfir"
    REAL, COMPLEX = 0, 1

    def __init__(self, kind_or_dtype, taps, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        self.kind = _parse_kind(kind_or_dtype, _REAL_COMPLEX, "RowFir")
        self._np = _row_type(self.kind)
        t = np.ascontiguousarray(taps, dtype=np.float32)
        first, p = _taps_ptr(t if t.ndim == 1 else t[0])
        capi.check(self._fn("create")(C.byref(self._h), device, self.kind, self.nchan, p, len(first), max_block), "qdsp_hip_rowfir_create")
        if t.ndim == 2:
            assert t.shape[0] == self.nchan, t.shape
            for c in range(1, self.nchan):
                self.set_taps(t[c], c)

    @classmethod
    def tile(cls) -> int:
        return int(capi.load().qdsp_hip_rowfir_tile())

    @classmethod
    def tap_group(cls) -> int:
        return int(capi.load().qdsp_hip_rowfir_tap_group())

    @property
    def ntaps(self) -> int:
        return capi.check(self._fn("ntaps")(self._h))

    def set_taps(self, taps, chan: int = -1):
        """chan -1: every channel, and the count may change (the history keeps its newest samples); chan >= 0: the same count."""
        t, p = _taps_ptr(taps)
        capi.check(self._fn("set_taps")(self._h, int(chan), p, len(t)), "qdsp_hip_rowfir_set_taps")

    def get_history(self, chan: int = 0) -> np.ndarray:
        n = self.ntaps - 1
        a = np.zeros(max(n, 1), dtype=self._np)
        capi.check(self._fn("get_history")(self._h, int(chan), a.ctypes.data))
        return a[:n]

    def set_history(self, hist, chan: int = 0):
        a = np.ascontiguousarray(hist, dtype=self._np)
        assert a.size == self.ntaps - 1, (a.size, self.ntaps)
        capi.check(self._fn("set_history")(self._h, int(chan), a.ctypes.data))


class DelayImag(_RowOp):
    """dsp::DelayImag (src/dsp/processing.h:300-344), the one-sample Q delay of offset PSK: out[i] = {x[i].re, x[i - 1].im}, bit
    copies, over `nchan` complex64 rows.  Entry points by input as for Squelch and Agc; `out` may not overlap the input."""

    _prefix = "qdsp_hip_delay_imag"
    _np = np.complex64

    def __init__(self, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, max_block), "qdsp_hip_delay_imag_create")

    def get_state(self, chan: int = 0) -> np.float32:
        """The carried lastIm, as the float32 it is (synchronises the device)."""
        v = C.c_float()
        capi.check(self._fn("get_state")(self._h, int(chan), C.byref(v)))
        return np.float32(v.value)

    def set_state(self, last_im: float, chan: int = -1):
        capi.check(self._fn("set_state")(self._h, int(chan), float(last_im)))


def rrc_taps(count: int, sample_rate: float, baud_rate: float, alpha: float) -> np.ndarray:
    """The taps FIR<complex_t> gets from dsp::RRCTaps (src/dsp/window.h:161-225): `count | 1` taps computed and normalised, the
    first `count` of them used.  Every step in the reference's types and order, as the C++ mirror's dsp/window.h computes it."""
    import math

    f32 = np.float32
    n = int(count) | 1
    centre = n // 2
    pi, a = float(FL_M_PI), f32(alpha)
    sps = float(f32(sample_rate) / f32(baud_rate))
    a4, om, op = float(f32(4) * a), float(f32(1) - a), float(f32(1) + a)
    taps, total = np.zeros(n, f32), 0.0
    for i in range(n):
        t = float(i - centre)
        arg = pi * t / sps
        edge = a4 * t / sps
        q = edge * edge - 1
        if abs(q) >= 0.000001:
            tail = math.sin(om * arg) / (a4 * t / sps) if i != centre else float(f32(f32(om) * FL_M_PI) / f32(a4))
            v = a4 * (math.cos(op * arg) + tail) / (q * pi)
        elif a == 1:
            v = -1.0
        else:
            lo, hi = om * arg, op * arg
            num = (math.sin(hi) * op * pi - math.cos(lo) * (float(f32(om) * FL_M_PI) * sps) / (a4 * t)
                   + math.sin(lo) * sps * sps / (a4 * t * t))
            v = a4 * num / (float(f32(f32(f32(-32) * FL_M_PI) * a) * a) * t / sps)
        taps[i] = f32(v)
        total += float(taps[i])
    for i in range(n):
        taps[i] = f32(float(taps[i]) / total)
    return taps[:int(count)].copy()


def _borrowed(cls, handle, **attrs):
    """A non-owning view of a stage handle of a chain with `cls`'s methods: closing it does nothing."""
    view = type("Borrowed" + cls.__name__, (cls,), {"close": lambda self: None})
    v = view.__new__(view)
    _Op.__init__(v)
    v._h = C.c_void_p(handle)
    for k, val in attrs.items():
        setattr(v, k, val)
    return v


class _Chain(_Counts, _RowOp):
    """What PskDemod and MskDemod share: a chain handle (include/qdsp_hip.h: PSKDemod and MSKDemod) runs every stage over `nchan`
    rows in one call with the intermediates on the device.  numpy input: the host entry point (one channel), returning the
    symbols; a 1-D tensor: *_process_dev; a 2-D one: `process_batch`, returning (rows, counts)."""

    _np = np.complex64

    def stage(self, which: int):
        """A non-owning view of stage `which` with that operator's methods (setters, getters, state); never process on it."""
        p = C.c_void_p()
        capi.check(self._fn("stage")(self._h, int(which), C.byref(p)), self._prefix + "_stage")
        return self._view(int(which), p.value)

    def tap(self, which: int, count: int = None):
        """The rows stage `which` wrote in the last call, as a (nchan, count) device tensor view (None where a later stage has
        overwritten them); valid until the next call."""
        import torch

        p, st = C.c_void_p(), C.c_int64()
        capi.check(self._fn("tap_dev")(self._h, int(which), C.byref(p), C.byref(st)), self._prefix + "_tap_dev")
        if not p.value:
            return None
        cplx = self._tap_complex(int(which))
        nfloat = self.nchan * st.value * (2 if cplx else 1)

        class _Holder:
            pass

        holder = _Holder()
        holder.__cuda_array_interface__ = {"shape": (nfloat,), "typestr": "<f4", "data": (p.value, False), "version": 2}
        t = torch.as_tensor(holder, device=f"cuda:{self.device}")
        t = torch.view_as_complex(t.view(self.nchan, st.value, 2)) if cplx else t.view(self.nchan, st.value)
        return t if count is None else t[:, :int(count)]

    def process_batch(self, x, out=None, count: int = None, counts=None):
        """Channel c = row c of the 2-D complex64 tensor `x` (rows may be padded).  Returns (rows, counts) as
        MmClockRecovery.process_batch does.  Asynchronous."""
        return self._batch(x, out, count, counts=counts)

    def _set_clock(self, clock, omega, gain_omega, mu_gain, rel_limit):
        par = [_per_chan(v, self.nchan) for v in (omega, gain_omega, mu_gain, rel_limit)]
        if any(np.any(v != v[0]) for v in par):
            clock._set_rows(par)   # (the order of MmClockRecovery.__init__: no step leaves the parameter rule)


class PskDemod(_Chain):
    """dsp::PSKDemod<ORDER, OFFSET> (src/dsp/demodulator.h:566-682): ComplexAgc (set point 1, max gain 65535) -> RowFir with the
    RRC taps -> CostasLoop of `order` -> DelayImag (`offset`) -> MmClockRecovery, over `nchan` complex64 rows in one call.
    Parameters are scalars or one value per channel.  The taps are `rrc_taps(rrc_tap_count, sample_rate, baud_rate, rrc_alpha)`
    per channel, the symbol period sample_rate / baud_rate in float.  `stage(PskDemod.AGC / RRC / COSTAS / DELAY / CLOCK)` gives
    the stage's own methods; `tap(which)` the rows it wrote in the last call."""

    _prefix = "qdsp_hip_psk"
    AGC, RRC, COSTAS, DELAY, CLOCK = 0, 1, 2, 3, 4

    def __init__(self, order: int, offset: bool, sample_rate, baud_rate, rrc_tap_count: int = 32, rrc_alpha=0.32, agc_rate=10e-4,
                 costas_bw=0.004, omega_gain=0.01 * 0.01 / 4, mu_gain=0.01, omega_rel_limit=0.005, nchan: int = 1, device: int = 0,
                 max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        self.order, self.offset = int(order), bool(offset)
        b = lambda v: _per_chan(v, self.nchan)   # noqa: E731
        sr, baud, alpha, rate, bw = b(sample_rate), b(baud_rate), b(rrc_alpha), b(agc_rate), b(costas_bw)
        taps = [rrc_taps(rrc_tap_count, sr[c], baud[c], alpha[c]) for c in range(self.nchan)]
        omega = (sr / baud).astype(np.float32)
        _, p = _taps_ptr(taps[0])
        go, gm, rl = b(omega_gain), b(mu_gain), b(omega_rel_limit)
        capi.check(self._fn("create")(C.byref(self._h), device, self.order, int(self.offset), self.nchan, max_block, p, len(taps[0]),
                                      float(rate[0]), float(bw[0]), float(omega[0]), float(go[0]), float(gm[0]), float(rl[0])),
                   "qdsp_hip_psk_create")
        rrc, agc, costas = self.stage(self.RRC), self.stage(self.AGC), self.stage(self.COSTAS)
        for c in range(1, self.nchan):
            if not np.array_equal(taps[c], taps[0]):
                rrc.set_taps(taps[c], c)
            if rate[c] != rate[0]:
                agc.set(1.0, 65535.0, float(rate[c]), c)
            if bw[c] != bw[0]:
                costas.set_bandwidth(float(bw[c]), c)
        self._set_clock(self.stage(self.CLOCK), omega, go, gm, rl)

    def _tap_complex(self, which: int) -> bool:
        return True

    def _view(self, which: int, handle):
        if which == self.AGC:
            return _borrowed(ComplexAgc, handle, nchan=self.nchan, device=self.device)
        if which == self.RRC:
            return _borrowed(RowFir, handle, nchan=self.nchan, device=self.device, kind=RowFir.COMPLEX, _np=np.complex64)
        if which == self.COSTAS:
            return _borrowed(CostasLoop, handle, nchan=self.nchan, device=self.device, order=self.order)
        if which == self.DELAY:
            return _borrowed(DelayImag, handle, nchan=self.nchan, device=self.device)
        return _borrowed(MmClockRecovery, handle, nchan=self.nchan, device=self.device, kind=1, _np=np.complex64)


class MskDemod(_Chain):
    """dsp::MSKDemod (src/dsp/demodulator.h:499-564): FmDemod (mono) -> MmClockRecovery on float rows, over `nchan` complex64 rows
    in one call; the symbols are float32.  Parameters are scalars or one value per channel.  The three loop parameters are
    forwarded (the reference's constructor drops them).  `stage(MskDemod.FM / CLOCK)`, `tap(MskDemod.FM)`."""

    _prefix = "qdsp_hip_msk"
    _out_np = np.float32
    FM, CLOCK = 0, 1

    def __init__(self, sample_rate, deviation, baud_rate, omega_gain=0.01 * 0.01 / 4, mu_gain=0.01, omega_rel_limit=0.005,
                 nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        b = lambda v: _per_chan(v, self.nchan)   # noqa: E731
        sr, dev, baud = b(sample_rate), b(deviation), b(baud_rate)
        omega = (sr / baud).astype(np.float32)
        go, gm, rl = b(omega_gain), b(mu_gain), b(omega_rel_limit)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, max_block, float(sr[0]), float(dev[0]), float(omega[0]),
                                      float(go[0]), float(gm[0]), float(rl[0])), "qdsp_hip_msk_create")
        fm = self.stage(self.FM)
        for c in range(1, self.nchan):
            if sr[c] != sr[0] or dev[c] != dev[0]:
                fm.set_fm(float(sr[c]), float(dev[c]), c)
        self._set_clock(self.stage(self.CLOCK), omega, go, gm, rl)

    def _tap_complex(self, which: int) -> bool:
        return False

    def _view(self, which: int, handle):
        if which == self.FM:
            return _borrowed(FmDemod, handle, nchan=self.nchan, device=self.device)
        return _borrowed(MmClockRecovery, handle, nchan=self.nchan, device=self.device, kind=0, _np=np.float32)


__all__ += ["RowFir", "DelayImag", "PskDemod", "MskDemod", "rrc_taps"]


class Threshold(_RowOp):
    """dsp::Threshold (src/dsp/processing.h:554-610): out = (in > 0.0f) as one uint8 per float32, `nchan` rows per launch
    (include/qdsp_hip.h: Threshold).  numpy input: the host entry point (one channel); a 1-D tensor: *_process_dev; a 2-D one:
    `process_batch`.  No state: `reset` does nothing."""

    _prefix = "qdsp_hip_threshold"
    _out_np = np.uint8
    _takes_in_counts = True

    def __init__(self, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        capi.check(self._fn("create")(C.byref(self._h), device, self.nchan, max_block), "qdsp_hip_threshold_create")

    @staticmethod
    def span() -> int:
        """Outputs per workgroup of threshold_kernel."""
        return int(capi.load().qdsp_hip_threshold_span())

    def reset(self):
        pass

    def out_size(self, n: int) -> int:
        return int(n)

    def process_batch(self, x, out=None, count: int = None, in_counts=None):
        """Channel c = row c of the 2-D float32 tensor `x` (rows may be padded).  `in_counts`: an int32 device tensor, row c
        converts min(max(in_counts[c], 0), count) floats and leaves the rest of its output row untouched.  Asynchronous."""
        return self._batch(x, out, count, in_counts=in_counts)


class Deframer(_Counts, _RowOp):
    """dsp::Deframer (src/dsp/deframing.h): finds `sync` (one bit per byte) in rows of one bit per byte, cuts frames of `frame_len`
    bits and packs them eight to a byte (include/qdsp_hip.h: Deframer).  `kind_or_dtype`: 0 / "bytes" / uint8 for uint8 rows,
    1 / "float" / float32 for float32 soft symbols thresholded on load.  `nchan` rows per launch, each with its own state.  A call
    of n bytes emits at most `out_size(n)` frames per row: `process` returns them as an (frames, frame_bytes) array (one row),
    `process_batch` the padded rows and the per-row frame counts."""

    _prefix = "qdsp_hip_deframer"
    _out_np = np.uint8
    _takes_in_counts = True
    BYTES, FLOAT = 0, 1

    def __init__(self, frame_len: int, sync, kind_or_dtype=0, nchan: int = 1, device: int = 0, max_block: int = 1_000_000):
        super().__init__()
        self.device = device
        self.nchan = int(nchan)
        self.kind = _parse_kind(kind_or_dtype, (("bytes", "uint8"), ("float", "float32")), "Deframer", exact=True)
        self._np = np.float32 if self.kind else np.uint8
        s = np.ascontiguousarray(sync, dtype=np.uint8).ravel()
        self.frame_len = int(frame_len)
        capi.check(self._fn("create")(C.byref(self._h), device, self.kind, self.nchan, max_block, self.frame_len, s.ctypes.data, s.size),
                   "qdsp_hip_deframer_create")
        self.sync_len = int(s.size)
        self._per = self.frame_bytes = int(self._fn("frame_bytes")(self._h))

    def _result(self, y):
        return y.reshape(y.shape[0] // self.frame_bytes, self.frame_bytes)

    @staticmethod
    def tile() -> int:
        """Positions per workgroup of deframe_match_kernel."""
        return int(capi.load().qdsp_hip_deframer_tile())

    @staticmethod
    def pack_span() -> int:
        """Positions per workgroup of deframe_pack_kernel (frame_len a multiple of 8)."""
        return int(capi.load().qdsp_hip_deframer_pack_span())

    def set_sync(self, sync):
        s = np.ascontiguousarray(sync, dtype=np.uint8).ravel()
        capi.check(self._fn("set_sync")(self._h, s.ctypes.data, s.size), "qdsp_hip_deframer_set_sync")

    def get_state(self, chan: int = 0):
        """(bits_read, bad, after) of one row: bits_read -1 = searching (synchronises the device)."""
        b, bad, aft = C.c_int(), C.c_int(), C.c_int()
        capi.check(self._fn("get_state")(self._h, int(chan), C.byref(b), C.byref(bad), C.byref(aft)), "qdsp_hip_deframer_get_state")
        return int(b.value), int(bad.value), bool(aft.value)

    def set_state(self, bits_read: int, bad: int, after: bool, chan: int = -1):
        capi.check(self._fn("set_state")(self._h, int(chan), int(bits_read), int(bad), int(bool(after))), "qdsp_hip_deframer_set_state")

    def process_batch(self, x, out=None, count: int = None, in_counts=None, counts=None):
        """Channel c = row c of the 2-D tensor `x` (rows may be padded: x.stride(0) >= count).  `in_counts`: an int32 device
        tensor of per-row input counts (what MmClockRecovery.process_batch or a chain returns), row c takes
        min(max(in_counts[c], 0), count) of its elements.  Returns (rows, counts): the (nchan, out_size(count) * frame_bytes) uint8
        view of `out`, row c's frames back to back in its first counts[c] * frame_bytes bytes and the rest untouched, and the
        frame counts as an int32 device tensor (`counts`, or a new one).  Asynchronous; `out` may not overlap `x`."""
        return self._batch(x, out, count, in_counts, counts)

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per call of `iters` back-to-back process_batch calls over the rows of the 2-D tensor `x` (HIP events on the
        launch stream).  The state moves on with every call."""
        import torch

        counts = torch.empty(self.nchan, dtype=torch.int32, device=x.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(int(iters)):
            self.process_batch(x, out, counts=counts)
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1)) / int(iters)


__all__ += ["Threshold", "Deframer"]
