"""How the library tells its per-row handles apart (qdsp_amd/csrc/stream_op.h: a table of the live handles' addresses, by kind),
asked of every per-row class of qdsp_amd.ops and qdsp_amd.fec through the C ABI: a live handle is taken by its own kind's entry
points and refused (QDSP_HIP_EINVAL) by every other kind's and sub-kind's; the shared entry points take all of them; host memory
that is no handle -- zeroed, or filled with a magic word of the scheme before the table -- a destroyed handle and a second destroy
are refused without being read; engine and channelizer handles are no per-row handles.  No kernel runs here: every call is an
`out_size` or a `process_dev` of no samples, on handles of one row and 64 samples.
"""
import ctypes as C
import inspect

import numpy as np
import pytest

from qdsp_amd import capi, fec, ops

pytestmark = pytest.mark.gpu

EINVAL = -10001
KW = dict(nchan=1, max_block=64)

# every per-row class, made as small as it goes (SsbDemod is one row by definition)
MAKE = {
    "FmDemod": lambda: ops.FmDemod(240000.0, 75000.0, **KW),
    "AmDemod": lambda: ops.AmDemod(**KW),
    "SsbDemod": lambda: ops.SsbDemod(48000.0, 3000.0, ops.SsbDemod.USB, max_block=64),
    "Deemp": lambda: ops.Deemp(48000.0, 50e-6, **KW),
    "Squelch": lambda: ops.Squelch(**KW),
    "Agc": lambda: ops.Agc(20.0, 48000.0, **KW),
    "StereoFmDemod": lambda: ops.StereoFmDemod(240000.0, 75000.0, pilot_taps=np.hanning(9).astype(np.float32), **KW),
    "FeedForwardAgc": lambda: ops.FeedForwardAgc(1, window=8, **KW),
    "ComplexAgc": lambda: ops.ComplexAgc(**KW),
    "CostasLoop": lambda: ops.CostasLoop(4, 0.01, **KW),
    "MmClockRecovery": lambda: ops.MmClockRecovery(1, 4.0, **KW),
    "RowFir": lambda: ops.RowFir(1, np.hanning(5).astype(np.float32), **KW),
    "DelayImag": lambda: ops.DelayImag(**KW),
    "PskDemod": lambda: ops.PskDemod(4, True, 4.0, 1.0, 9, **KW),
    "MskDemod": lambda: ops.MskDemod(4.0, 1.0, 1.0, **KW),
    "Threshold": lambda: ops.Threshold(**KW),
    "Deframer": lambda: ops.Deframer(16, np.array([1, 0, 1, 1], np.uint8), 0, **KW),
    "RsDecoder": lambda: fec.RsDecoder(0x11d, 1, 1, 4, **KW),
    "FalconRs": lambda: fec.FalconRs(**KW),
}
# the cheap entry point of each kind and sub-kind (by the prefix of its C names): no kernel, no device work
OUT_SIZE = ("qdsp_hip_ffagc", "qdsp_hip_mmcr", "qdsp_hip_psk", "qdsp_hip_msk", "qdsp_hip_deframer", "qdsp_hip_rs")
# the magic words the eleven older kinds carried at offset 0 until the table took over (stream_op.h of the parent commit)
OLD_MAGICS = {"QDMD": 0x51444d44, "QDEE": 0x51444545, "QLVL": 0x514c564c, "QSFM": 0x5153464d, "QFAG": 0x51464147, "QCAG": 0x51434147,
              "QCOS": 0x51434f53, "QMMC": 0x514d4d43, "QRFI": 0x51524649, "QDIM": 0x5144494d, "QPSK": 0x5150534b}


def probe(L, prefix, h):
    """The kind's cheap entry point on h: >= 0 if it takes the handle, QDSP_HIP_EINVAL if it refuses it."""
    if prefix in OUT_SIZE:
        return int(getattr(L, prefix + "_out_size")(h, 1))
    return int(getattr(L, prefix + "_process_dev")(h, None, 0, None, None))


def last_kernel(L, h):
    name = C.create_string_buffer(64)
    return int(L.qdsp_hip_last_kernel(h, name, 64, None, None, None))


def timed(L, h):
    """One timed call of no samples: 0 from a handle whatever its kind, QDSP_HIP_EINVAL from what is none."""
    ms = C.c_float(-1.0)
    return int(L.qdsp_hip_time_process_dev(h, None, 0, None, None, 1, C.byref(ms)))


@pytest.fixture(scope="module")
def L():
    import torch

    assert torch.cuda.is_available()
    return capi.load()


@pytest.fixture(scope="module")
def live(L):
    made = {name: make() for name, make in MAKE.items()}
    yield made
    for op in made.values():
        op.close()


@pytest.fixture(scope="module")
def prefixes(live):
    return sorted({op._prefix for op in live.values()})


def test_every_per_row_class_is_here():
    """A new per-row class has to be added to MAKE; the classes share 17 prefixes: fourteen kinds, and a second sub-kind each of
    Level (Squelch / Agc), Demod (SsbDemod against the other demodulators) and the chain (PskDemod / MskDemod)."""
    rows = {n for mod in (ops, fec) for n in mod.__all__ if inspect.isclass(getattr(mod, n)) and issubclass(getattr(mod, n), ops._Rows)}
    assert rows == set(MAKE)
    assert len({getattr(mod, n)._prefix for mod in (ops, fec) for n in mod.__all__ if n in rows}) == 17


@pytest.mark.parametrize("name", sorted(MAKE))
def test_a_live_handle_is_taken_by_its_own_kind_only(L, live, prefixes, name):
    op = live[name]
    for p in prefixes:
        rc = probe(L, p, op._h)
        assert (rc >= 0) if p == op._prefix else (rc == EINVAL), (name, p, rc)


@pytest.mark.parametrize("name", sorted(MAKE))
def test_the_shared_entry_points_take_every_kind(L, live, name):
    h = live[name]._h
    assert last_kernel(L, h) == 0
    assert L.qdsp_hip_set_done_event(h, None) == 0
    assert timed(L, h) == 0


def test_host_memory_that_is_no_handle_is_refused(L, prefixes):
    """256 bytes of zeros, and the same filled with each magic word of the older scheme: junk host memory, which every entry
    point refuses by its address."""
    for tag, word in [("zeros", 0)] + sorted(OLD_MAGICS.items()):
        junk = (C.c_uint32 * 64)(*([word] * 64))
        for p in prefixes:
            assert probe(L, p, junk) == EINVAL, (tag, p)
        assert last_kernel(L, junk) == EINVAL and L.qdsp_hip_set_done_event(junk, None) == EINVAL and timed(L, junk) == EINVAL, tag
        assert all(v == word for v in junk), tag


@pytest.mark.parametrize("name", sorted(MAKE))
def test_a_destroyed_handle_is_refused_and_a_second_destroy_does_nothing(L, live, name):
    op = MAKE[name]()
    prefix, old = op._prefix, C.c_void_p(op._h.value)
    assert probe(L, prefix, old) >= 0 and last_kernel(L, old) == 0
    op.close()
    assert probe(L, prefix, old) == EINVAL and last_kernel(L, old) == EINVAL       # (looked up by address: the freed handle is not read)
    assert getattr(L, prefix + "_destroy")(old) is None
    assert probe(L, prefix, old) == EINVAL
    assert probe(L, prefix, live[name]._h) >= 0                                     # the kind's other handle has not noticed


def test_engine_and_channelizer_handles_are_no_per_row_handles(L, prefixes):
    fir = ops.Fir(np.hanning(9).astype(np.float32), max_block=64)
    incs = [ops.phase_delta(1.0, -(c - 3.5) / 8.0) for c in range(8)]
    chan = ops.Channelizer(np.hanning(32).astype(np.float32), 1, 8, incs, max_block=0)
    for h in (fir._h, chan._h):
        for p in prefixes:
            assert probe(L, p, h) == EINVAL, p
        assert last_kernel(L, h) == 0
    fir.close()
    chan.close()
