"""Forward error correction on the GPU: the Reed-Solomon decoder over rows of interleaved frames and its FalconRS preset
(include/qdsp_hip.h: Reed-Solomon decoder and FalconRS), on the per-row operators' plumbing of qdsp_amd.ops.  Every count here is
in frames.  There is no fallback: the decode runs in rs_decode_kernel or raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import capi
from .ops import _Counts, _in_counts_ptr, _is_torch, _RowOp

__all__ = ["RsDecoder", "FalconRs", "ccsds_dual_basis", "ccsds_randomizer"]

CCSDS_POLY = 0x187


def _gf_tables(poly: int):
    exp, log = np.zeros(512, np.uint8), np.zeros(256, np.uint8)
    e = 1
    exp[0] = 1
    for i in range(1, 512):
        e <<= 1
        if e > 255:
            e ^= poly
        exp[i] = e
        if i < 256:
            log[e] = i
    return exp, log


def ccsds_randomizer() -> np.ndarray:
    """The 255 bytes of the CCSDS pseudo-randomiser: s[n + 8] = s[n] ^ s[n + 3] ^ s[n + 5] ^ s[n + 7] from eight ones, MSB first."""
    s = np.ones(255 * 8, np.uint8)
    for n in range(255 * 8 - 8):
        s[n + 8] = s[n] ^ s[n + 3] ^ s[n + 5] ^ s[n + 7]
    return np.packbits(s)


def ccsds_dual_basis():
    """(to_db, from_db), 256 bytes each: bit (7 - j) of to_db[x] is Tr(alpha^(117 j mod 255) x) over the field of 0x187, with
    Tr(y) = y + y^2 + ... + y^128; from_db is its inverse."""
    exp, log = _gf_tables(CCSDS_POLY)
    ie, il = exp.astype(np.int64), log.astype(np.int64)

    def mul(a, b):
        return np.where((a != 0) & (b != 0), exp[il[a] + il[b]], 0).astype(np.uint8)

    x = np.arange(256).astype(np.uint8)
    to_db = np.zeros(256, np.uint8)
    for j in range(8):
        y = mul(np.full(256, ie[(117 * j) % 255], np.uint8), x)
        tr = np.zeros(256, np.uint8)
        for _ in range(8):
            tr ^= y
            y = mul(y, y)
        to_db |= ((tr & 1) << (7 - j)).astype(np.uint8)
    from_db = np.zeros(256, np.uint8)
    from_db[to_db] = x
    return to_db, from_db


def _table(v, what: str, size: int = None):
    if v is None:
        return None
    a = np.ascontiguousarray(v)
    if a.dtype != np.uint8 or a.ndim != 1 or (size is not None and a.size != size):
        raise ValueError(f"{what}: {'uint8 bytes' if size is None else f'{size} uint8 bytes'}, not {a.dtype} of shape {a.shape}")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


class RsDecoder(_Counts, _RowOp):
    """Reed-Solomon decoding of frames of `depth` interleaved RS(255, 255 - num_roots) codewords behind `skip` bytes, libcorrect's
    correct_reed_solomon_decode bit for bit; a frame with a codeword that does not decode is dropped.  `in_map` / `out_map`: 256
    bytes applied to every input / output byte; `xor`: bytes XOR-ed onto the output, repeating; `full_out`: a frame comes out
    255 * depth bytes long, zeros (mapped and XOR-ed) behind the message bytes, as the reference's FalconRS leaves them.
    numpy input (whole frames, one row): the host entry point, returns the good frames as (good, frame_out); a 1-D tensor:
    *_process_dev; a 2-D tensor of `nchan` rows: `process_batch`."""

    _prefix = "qdsp_hip_rs"
    _np = np.uint8
    _out_np = np.uint8
    _takes_in_counts = True

    def __init__(self, prim_poly: int, first_root: int, root_gap: int, num_roots: int, depth: int = 1, skip: int = 0, full_out: bool = False,
                 in_map=None, out_map=None, xor=None, nchan: int = 1, device: int = 0, max_block: int = 4096):
        prim_poly, first_root, root_gap, num_roots, depth, skip = (int(v) for v in (prim_poly, first_root, root_gap, num_roots, depth, skip))
        if not 0x100 <= prim_poly <= 0x1ff:
            raise ValueError(f"prim_poly: 9 bits (degree 8), not {prim_poly:#x}")
        if not 0 <= first_root <= 255:
            raise ValueError(f"first_root: 0 .. 255, not {first_root}")
        if not 1 <= root_gap <= 254 or math.gcd(root_gap, 255) != 1:
            raise ValueError(f"root_gap: coprime to 255, not {root_gap}")
        if not 2 <= num_roots <= 32:
            raise ValueError(f"num_roots: 2 .. 32, not {num_roots}")
        if not 1 <= depth <= 8:
            raise ValueError(f"depth: 1 .. 8, not {depth}")
        if not 0 <= skip <= 64:
            raise ValueError(f"skip: 0 .. 64, not {skip}")
        im, om, xr = _table(in_map, "in_map", 256), _table(out_map, "out_map", 256), _table(xor, "xor")
        if xr is not None and not 1 <= xr.size <= 255 * depth:
            raise ValueError(f"xor: 1 .. {255 * depth} bytes, not {xr.size}")
        self._setup(nchan, device)
        rc = self._fn("create")(C.byref(self._h), device, self.nchan, int(max_block), prim_poly, first_root, root_gap, num_roots, depth, skip,
                                int(bool(full_out)), _ptr(im), _ptr(om), _ptr(xr), 0 if xr is None else xr.size)
        capi.check(rc, "qdsp_hip_rs_create")      # (a polynomial that is not primitive is the library's to refuse)
        self._sizes()

    def _setup(self, nchan, device):
        _RowOp.__init__(self)
        self.device = device
        self.nchan = int(nchan)

    def _sizes(self):
        self.frame_in = int(self._fn("frame_in_bytes")(self._h))
        self._per = self.frame_out = int(self._fn("frame_out_bytes")(self._h))

    def reset(self):
        pass                                      # no state between frames

    def set_maps(self, in_map=None, out_map=None, xor=None):
        """Replace the two maps and the XOR sequence (None: the identity / none).  Synchronises; acts from the next call."""
        im, om, xr = _table(in_map, "in_map", 256), _table(out_map, "out_map", 256), _table(xor, "xor")
        capi.check(self._fn("set_maps")(self._h, _ptr(im), _ptr(om), _ptr(xr), 0 if xr is None else xr.size), "qdsp_hip_rs_set_maps")

    def _result(self, y):
        return y.reshape(y.shape[0] // self.frame_out, self.frame_out)

    def _whole_frames(self, nbytes: int) -> int:
        if nbytes % self.frame_in:
            raise ValueError(f"whole frames of {self.frame_in} bytes, not {nbytes} bytes")
        return nbytes // self.frame_in

    def process(self, x, out=None):
        if _is_torch(x):
            return self.process_batch(x, out)[0] if x.dim() == 2 else self._process_dev(x, out)
        a = np.ascontiguousarray(x, dtype=np.uint8).ravel()
        n = self._whole_frames(a.size)
        y = np.empty(max(n, 1) * self.frame_out, np.uint8)
        rc = capi.check(self._fn("process")(self._h, a.ctypes.data, n, y.ctypes.data), "qdsp_hip_rs_process")
        return self._result(y[:rc * self.frame_out])

    def _process_dev(self, x, out=None):
        import torch

        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.uint8 and x.dim() == 1 and self.nchan == 1, "one contiguous row"
        n = self._whole_frames(x.numel())
        if out is None:
            out = torch.empty(max(n, 1) * self.frame_out, dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.uint8 and out.numel() >= n * self.frame_out
        stream = torch.cuda.current_stream(x.device).cuda_stream
        capi.check(int(self._fn("process_dev")(self._h, x.data_ptr(), n, out.data_ptr(), stream)), "qdsp_hip_rs_process_dev")
        return self._result(out[:int(self.counts()[0]) * self.frame_out])

    def process_batch(self, x, out=None, nframes: int = None, in_counts=None, counts=None, errs=None):
        """Channel c = row c of the 2-D uint8 tensor `x`, frames back to back (rows may be padded and start at any byte).
        `in_counts`: an int32 device tensor of per-row frame counts (what Deframer.process_batch returns).  Returns (rows, counts):
        the (nchan, nframes * frame_out) view of `out`, row c's good frames back to back in its first counts[c] slots and the rest
        untouched, and the good-frame counts as an int32 device tensor.  `errs`: an int32 device tensor (nchan, nframes * depth)
        that receives per codeword -1 or the symbols corrected.  Asynchronous; `out` may not overlap `x`."""
        import torch

        assert x.is_cuda and x.dtype == torch.uint8 and x.dim() == 2 and x.shape[0] == self.nchan and (x.shape[1] <= 1 or x.stride(1) == 1)
        n = x.shape[1] // self.frame_in if nframes is None else int(nframes)
        assert 0 <= n * self.frame_in <= x.shape[1]
        if out is None:
            out = torch.empty((self.nchan, max(n, 1) * self.frame_out), dtype=torch.uint8, device=x.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == self.nchan and out.shape[1] >= n * self.frame_out
        assert out.shape[1] <= 1 or out.stride(1) == 1
        if counts is None:
            counts = torch.empty(self.nchan, dtype=torch.int32, device=x.device)
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == self.nchan
        ep = None
        if errs is not None:
            assert errs.is_cuda and errs.dtype == torch.int32 and errs.is_contiguous() and errs.numel() >= self.nchan * n * (self.frame_in // 255)
            ep = errs.data_ptr()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = self._fn("process_batch_dev")(self._h, x.data_ptr(), n, x.stride(0), _in_counts_ptr(in_counts, self.nchan, x.device), out.data_ptr(),
                                           out.stride(0), counts.data_ptr(), ep, stream)
        capi.check(int(rc), "qdsp_hip_rs_process_batch_dev")
        return out[:, :n * self.frame_out], counts

    def time_dev(self, x, out, iters: int) -> float:
        """Mean ms per call of `iters` back-to-back process_batch calls over the rows of the 2-D tensor `x`."""
        import torch

        counts = torch.empty(self.nchan, dtype=torch.int32, device=x.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(int(iters)):
            self.process_batch(x, out, counts=counts)
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1)) / int(iters)


class FalconRs(RsDecoder):
    """dsp::FalconRS (src/dsp/falcon_fec.h): frames of a 4-byte sync word and five interleaved CCSDS RS(255, 239) codewords in the
    dual basis come out as 1275 de-randomised bytes; a frame with a codeword that does not decode is dropped."""

    def __init__(self, nchan: int = 1, device: int = 0, max_block: int = 4096):
        self._setup(nchan, device)
        capi.check(self._L.qdsp_hip_falcon_rs_create(C.byref(self._h), device, self.nchan, int(max_block)), "qdsp_hip_falcon_rs_create")
        self._sizes()
