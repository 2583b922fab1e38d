"""What the PSKDemod / MSKDemod tests share: DelayImag's definition, the numpy chain built from the definitions the stage tests
already use (cagc_ref, the k-ordered FIR, costas_ref, mm_ref), a PSK signal generator, and the convergence condition that the CPU
test asserts on the numpy chain and the GPU test on the operator."""
import math

import numpy as np

import _mmcr_ref as M
from _numerics import direct_fma32
from test_cagc_cpu import cagc_ref
from test_costas_cpu import costas_gains, costas_ref

F32 = np.float32


# ---- DelayImag ----
def delay_imag_ref(x, last_im=0.0):
    """DelayImag::run over one call (processing.h:321-336): (out, lastIm).  Bit copies: the parts are moved as float32 words."""
    x = np.ascontiguousarray(x, np.complex64)
    w = x.view(np.uint32).reshape(-1, 2)
    out = np.empty_like(w)
    out[:, 0] = w[:, 0]
    last = np.asarray(last_im, F32).reshape(1).view(np.uint32)[0]
    if len(w):
        out[0, 1] = last
        out[1:, 1] = w[:-1, 1]
        last = w[-1, 1]
    return out.reshape(-1).view(np.complex64), np.asarray([last], np.uint32).view(F32)[0]


# ---- the numpy chain ----
def psk_chain_ref(x, order, offset, taps, agc_rate=F32(10e-4), costas_bw=0.004, omega=4.0, gain_omega=0.01 * 0.01 / 4, mu_gain=0.01,
                  rel_limit=0.005):
    """One row, one call from the state after create: PSKDemod::init's parameters, every stage the reference's float code
    (mm_ref: its interpolator sum in FP64).  Returns (symbols, the Costas loop's final frequency, the stage outputs)."""
    a, _ = cagc_ref(x, 1.0, 65535.0, agc_rate)
    f = direct_fma32(taps, a)
    alpha, beta = costas_gains(costas_bw)
    c, freq, _ = costas_ref(f, order, alpha, beta)
    d = delay_imag_ref(c)[0] if offset else c
    y, _ = M.mm_ref(d, 1, M.params(omega, gain_omega, mu_gain, rel_limit))
    return y, float(np.asarray(freq).reshape(-1)[0]), {"agc": a, "rrc": f, "costas": c, "delay": d}


# ---- the generator ----
def rrc_pulse(t, alpha):
    """The root-raised-cosine pulse of unit symbol period at times t (in symbols), FP64, its removable singularities filled in."""
    t = np.asarray(t, np.float64)
    out = np.empty_like(t)
    zero = np.abs(t) < 1e-9
    edge = np.abs(np.abs(4 * alpha * t) - 1) < 1e-9
    reg = ~(zero | edge)
    tr = t[reg]
    out[reg] = (np.sin(np.pi * tr * (1 - alpha)) + 4 * alpha * tr * np.cos(np.pi * tr * (1 + alpha))) / (np.pi * tr * (1 - (4 * alpha * tr) ** 2))
    out[zero] = 1 - alpha + 4 * alpha / np.pi
    out[edge] = alpha / math.sqrt(2) * ((1 + 2 / np.pi) * math.sin(np.pi / (4 * alpha)) + (1 - 2 / np.pi) * math.cos(np.pi / (4 * alpha)))
    return out


SPAN = 10                   # the transmit pulse is cut at +-SPAN symbols


def psk_signal(order, nsym, sps=4.0, alpha=0.32, seed=1, rms=0.05, carrier=2e-3, phase=0.7, timing=0.37, noise=0.05):
    """(samples complex64, sent symbols complex128): `order`-PSK symbols (2: +-1; 4: (+-1 +-j) / sqrt 2) through a root-raised-cosine
    pulse at `sps` samples per symbol, delayed by the fraction `timing` of a sample, scaled to the RMS amplitude `rms`, turned by
    `carrier` rad per sample from `phase`, plus complex noise of `noise` times the signal's RMS."""
    assert order in (2, 4)
    rng = np.random.default_rng(seed)
    if order == 2:
        sym = (rng.integers(0, 2, nsym) * 2 - 1).astype(np.complex128)
    else:
        sym = ((rng.integers(0, 2, nsym) * 2 - 1) + 1j * (rng.integers(0, 2, nsym) * 2 - 1)) / math.sqrt(2)
    n = int(nsym * sps)
    pos = (np.arange(n, dtype=np.float64) - timing) / sps            # in symbols: symbol k sits at pos == k
    k0 = np.rint(pos).astype(np.int64)
    x = np.zeros(n, np.complex128)
    for j in range(-SPAN, SPAN + 1):
        k = k0 + j
        ok = (k >= 0) & (k < nsym)
        x += np.where(ok, sym[np.clip(k, 0, nsym - 1)] * rrc_pulse(pos - k, alpha), 0)
    x *= rms / math.sqrt(np.mean(np.abs(x) ** 2))
    x *= np.exp(1j * (carrier * np.arange(n) + phase))
    x += noise * rms * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)
    return x.astype(np.complex64), sym


# ---- the condition ----
CARRIER, FREQ_WINDOW, TAIL = 2e-3, 5e-4, 250


def decision_errors(y, sent, order):
    """The fewest decision errors over the second half of the sent symbols less the last TAIL, over the rotations of the
    constellation and delays of -16 .. 16 symbols: (errors, compared, rotation, delay).  Symbol j of y is compared with sent[j - d]."""
    y = np.asarray(y, np.complex128)
    nsym = len(sent)
    lo, hi = nsym // 2, nsym - TAIL
    best = None
    for rot in range(order):
        z = y * np.exp(-2j * np.pi * rot / order)
        if order == 2:
            dec = np.sign(z.real).astype(np.complex128)
        else:
            dec = (np.sign(z.real) + 1j * np.sign(z.imag)) / math.sqrt(2)
        for d in range(-16, 17):
            j = np.arange(lo, hi) + d
            if j.min() < 0 or j.max() >= len(dec):
                continue
            err = int(np.count_nonzero(np.abs(dec[j] - sent[lo:hi]) > 1e-6))
            if best is None or err < best[0]:
                best = (err, hi - lo, rot, d)
    assert best is not None, "too few symbols came out"
    return best


def converged(y, freq, sent, order):
    """The convergence condition: (ok, report)."""
    err, n, rot, d = decision_errors(y, sent, order)
    rep = dict(errors=err, compared=n, rotation=rot, delay=d, freq=float(freq))
    return err == 0 and abs(float(freq) - CARRIER) <= FREQ_WINDOW, rep
