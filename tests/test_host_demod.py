"""The demodulator blocks of the C++ mirror (qdsp_amd/host/dsp/demodulator.h) inside source -> VFO -> demodulator -> sink
graphs (qdsp_amd/host/build/demod_check), with the VFO -> demodulator link on the device and on the host: what comes out equals
the restatement of src/dsp/demodulator.h (tests/test_demod_cpu.py) applied to the VFO's own output."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from qdsp_amd import ops
from test_demod_cpu import _same_bits, am_mag, fm_ref, phasor_speed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "qdsp_amd", "host")
BIN = os.path.join(HOST, "build", "demod_check")
N, BLOCK, DECIM = 240_000, 24_000, 10
VFO_ARGS = ["300000", "2400000", "240000", "200000"]    # offset, inSR, outSR, bandwidth: 2.4 Msps -> 240 ksps


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL, timeout=300)
    d = tmp_path_factory.mktemp("demodgraph")
    O.synth_iq(0, N, seed=42).tofile(d / "x.cf32")
    subprocess.run([BIN, "vfo", str(d / "x.cf32"), str(d / "v.cf32"), str(BLOCK)] + VFO_ARGS, check=True, timeout=180,
                   capture_output=True, text=True)
    v = np.fromfile(d / "v.cf32", dtype=np.complex64)
    assert len(v) == N // DECIM
    return d, v


def run(d, mode, link, *params):
    out = d / f"{mode}_{link}.bin"
    r = subprocess.run([BIN, mode, link, str(d / "x.cf32"), str(out), str(BLOCK)] + VFO_ARGS + [str(p) for p in params],
                       check=True, timeout=180, capture_output=True, text=True)
    assert "graph ok" in r.stdout and f"{link if link == 'host' else 'device'} link" in r.stdout
    return out


@pytest.mark.parametrize("link", ["dev", "host"])
def test_fm_blocks(graph, link):
    d, v = graph
    want, _ = fm_ref(v, phasor_speed(240_000.0, 75_000.0))
    y = np.fromfile(run(d, "fm", link, 75_000), dtype=np.float32)
    assert _same_bits(y, want)
    ys = np.fromfile(run(d, "fms", link, 75_000), dtype=np.float32).reshape(-1, 2)
    assert _same_bits(ys[:, 0], want) and _same_bits(ys[:, 1], want)


@pytest.mark.parametrize("link", ["dev", "host"])
def test_am_block(graph, link):
    d, v = graph
    y = np.fromfile(run(d, "am", link), dtype=np.float32)
    vb = BLOCK // DECIM
    assert len(y) == len(v)
    for a in range(0, len(v), vb):          # one run() per VFO output block: each subtracts its own mean
        m = am_mag(v[a:a + vb])
        mu = np.mean(m.astype(np.float64))
        assert np.max(np.abs(y[a:a + vb].astype(np.float64) - (m - mu))) <= 2 * np.spacing(np.max(m))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("link", ["dev", "host"])
def test_ssb_block(graph, link, mode):
    d, v = graph
    y = np.fromfile(run(d, "ssb", link, 10_000, mode), dtype=np.float32)
    xl = ops.Xlator(phase_inc=ops.ssb_phase_delta(240_000.0, 10_000.0, mode))
    vb = BLOCK // DECIM
    want = np.concatenate([xl.process(v[a:a + vb]).real for a in range(0, len(v), vb)])
    assert _same_bits(y, want)


def test_set_input_on_a_running_block(graph):
    """setInput() of detail::hip_block (dsp/hip_block.h) on a live Squelch: source A (1+0j) -> Squelch -> sink, moved to source B
    (2+0j) after 8 blocks of 4 096, 8 more blocks of B.  The harness fails on a block that mixes the two, on a block of A after one
    of B, and on a sample that is neither."""
    r = subprocess.run([BIN, "rebind", "4096", "8", "8"], check=True, timeout=60, capture_output=True, text=True)
    assert "graph ok" in r.stdout, r.stdout + r.stderr
