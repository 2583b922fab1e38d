"""Shared numerics helpers for tests/test_numerics_cpu.py and tests/test_gpu_numerics.py (imported like conftest).

Three pieces:
  * signal generators, computed in FP64 and rounded to complex64 / float32 at the end;
  * FP64 references returned as float64 / complex128 (the oracle returns float32, and that rounding would hide errors below
    ~1e-12, where the quiet-region floor of a -100 dB tone sits);
  * FP32 yardsticks -- the error an honest FP32 implementation makes on the same input -- and a region metric: per region,
    the RMS and the max of |y - ref|, bounded by K x the yardstick's error in that region plus a tiny absolute floor.
"""
import numpy as np

K = 8.0            # a kernel may be this many times worse than the FP32 yardstick of its family, region by region
FLOOR = 1e-30      # absolute floor of the region bound (an exactly zero yardstick error in an all-zero region)


# ------------------------------------------------------------------------------------------------ signal generators
def tone(n, f, amp=1.0, t0=0, phase=0.0, real=False):
    """amp exp(j (2 pi f t + phase)) for t = t0 .. t0 + n - 1 (f in cycles per sample); real: amp cos(...)."""
    t = np.arange(t0, t0 + n, dtype=np.float64)
    arg = 2.0 * np.pi * ((f * t) % 1.0) + phase
    return amp * np.cos(arg) if real else amp * np.exp(1j * arg)


def gate(x, start, stop):
    """x with every sample outside [start, stop) set to zero (a burst)."""
    y = np.array(x, copy=True)
    y[:start] = 0
    y[stop:] = 0
    return y


def dc(n, amp=1.0, real=False):
    return np.full(n, amp, np.float64) if real else np.full(n, amp + 0j, np.complex128)


def bin_tone(n, k, N, amp=1.0, real=False):
    """A tone centred on bin k of an N-point transform."""
    return tone(n, k / N, amp, real=real)


def nyquist(n, amp=1.0, real=False):
    y = amp * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    return y if real else y.astype(np.complex128)


def to32(x):
    """Round an FP64 signal to the kernels' sample type: complex64, or float32 for real data."""
    x = np.asarray(x)
    return np.ascontiguousarray(x.astype(np.complex64 if np.iscomplexobj(x) else np.float32))


def blocker_stream(n, loud_end, f_block, f_weak, weak_db=-100.0, real=False, seed=0):
    """A 0 dBFS out-of-band blocker on [0, loud_end) plus a weak in-band tone throughout (FP64, not rounded)."""
    ph = np.random.default_rng(seed).uniform(0, 2 * np.pi, 2)
    x = gate(tone(n, f_block, 1.0, phase=ph[0], real=real), 0, loud_end)
    return x + tone(n, f_weak, 10.0 ** (weak_db / 20.0), phase=ph[1], real=real)


# ------------------------------------------------------------------------------------------------ FP64 references
def fir_ref64(taps, x, hist=None):
    """FIR<T> (filter.h): y[i] = sum_k h[k] buf[i + k], buf = [hist (ntaps - 1) | x], in FP64 on the f32-rounded data."""
    h = np.asarray(taps, np.float32).astype(np.float64)
    xd = np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if hist is None:
        hist = np.zeros(len(h) - 1, xd.dtype)
    buf = np.concatenate([np.asarray(hist).astype(xd.dtype), xd])
    return np.convolve(buf, h[::-1], mode="valid")


def build_phases64(taps, L):
    """buildTapPhases (resampling.h): phases[(L - 1) - p][t] = taps[t L + p], zero past the prototype."""
    h = np.asarray(taps, np.float32).astype(np.float64)
    tpp = -(-len(h) // L)
    ph = np.zeros((L, tpp))
    hp = np.concatenate([h, np.zeros(tpp * L - len(h))])
    for p in range(L):
        ph[(L - 1) - p] = hp[p::L]
    return ph


class Resampler64:
    """PolyphaseResampler<T>::run restated in FP64, call by call like oracle.Resampler: buffer = [hist (tpp) | in],
    out[o] = dot(buffer[i / L ..], phases[i % L]) with i = o M restarting at 0 on every call, hist' = the buffer's tail."""

    def __init__(self, taps, L, M, complex_data=True):
        self.L, self.M = int(L), int(M)
        self.ph = build_phases64(taps, self.L)
        self.tpp = self.ph.shape[1]
        self.dt = np.complex128 if complex_data else np.float64
        self.hist = np.zeros(self.tpp, self.dt)

    def process(self, x):
        xd = np.asarray(x).astype(self.dt)
        n = len(xd)
        buf = np.concatenate([self.hist, xd])
        nout = n * self.L // self.M
        y = np.zeros(nout, self.dt)
        if self.L == 1:
            h = self.ph[0]
            for j in range(self.tpp):
                y += h[j] * buf[j: j + self.M * nout: self.M][:nout]
        else:
            i = np.arange(nout, dtype=np.int64) * self.M
            st, p = i // self.L, i % self.L
            for j in range(self.tpp):
                y += self.ph[p, j] * buf[st + j]
        self.hist = buf[n: n + self.tpp].copy()
        return y

    def windows(self, n, start):
        """Stream positions [first, last] of each output's window, for a call of n samples beginning at stream position start."""
        nout = n * self.L // self.M
        i = np.arange(nout, dtype=np.int64) * self.M
        first = start - self.tpp + i // self.L
        return first, first + self.tpp - 1


def run_calls(op_process, x, sizes):
    """One stream through a stateful process() in calls of the given sizes (the last one takes the rest)."""
    out, a = [], 0
    for s in list(sizes) + [len(x)]:
        b = min(len(x), a + s)
        if b > a:
            out.append(op_process(x[a:b]))
        a = b
        if a >= len(x):
            break
    return np.concatenate(out)


def call_cuts(n, sizes):
    cuts, a = [0], 0
    for s in list(sizes) + [n]:
        a = min(n, a + s)
        if a > cuts[-1]:
            cuts.append(a)
        if a >= n:
            break
    return cuts


def stream_windows(taps, L, M, cuts, fir=False):
    """[first, last] input positions of every output's window over a stream cut into calls at `cuts`: a resampler's
    (tpp samples of history, output o of a call ends its window at start + o M / L - 1), or a FIR's (fir=True: output i
    ends its window at sample i)."""
    r = Resampler64(taps, L, M)
    f, l = [], []
    for a, b in zip(cuts, cuts[1:]):
        w0, w1 = r.windows(b - a, a)
        f.append(w0 + (1 if fir else 0))
        l.append(w1 + (1 if fir else 0))
    return np.concatenate(f), np.concatenate(l)


def _hist(h, x32, hist, resamp):
    if hist is None:
        hist = np.zeros(len(h) - (0 if resamp else 1), x32.dtype)
    return np.concatenate([np.asarray(hist, x32.dtype), x32])


# ------------------------------------------------------------------------------------------------ FP32 yardsticks
def fft_radix2(x, twiddle_bits=None, inverse=False):
    """Iterative radix-2 DIT FFT over the last axis in complex64 (numpy vector ops), with its twiddles optionally rounded
    to `twiddle_bits` mantissa bits -- the broken-model control of the overlap-save yardstick."""
    x = np.asarray(x, np.complex64)
    N = x.shape[-1]
    lg = N.bit_length() - 1
    assert 1 << lg == N
    rev = np.zeros(N, np.int64)
    for b in range(lg):
        rev |= ((np.arange(N) >> b) & 1) << (lg - 1 - b)
    a = x[..., rev].copy()
    sgn = 1.0 if inverse else -1.0
    m = 1
    while m < N:
        k = np.arange(m)
        w = np.exp(sgn * 1j * np.pi * k / m)
        if twiddle_bits is not None:
            w = round_mantissa(w.real, twiddle_bits) + 1j * round_mantissa(w.imag, twiddle_bits)
        w = w.astype(np.complex64)
        a = a.reshape(a.shape[:-1] + (N // (2 * m), 2, m))
        t = a[..., 1, :] * w
        u = a[..., 0, :]
        a = np.stack([u + t, u - t], axis=-2).reshape(a.shape[:-3] + (N,))
        m *= 2
    return a / np.float32(N) if inverse else a


def round_mantissa(v, bits):
    """v rounded to `bits` bits of mantissa (FP64 in, FP64 out)."""
    m, e = np.frexp(np.asarray(v, np.float64))
    return np.ldexp(np.round(m * (1 << bits)) / (1 << bits), e)


def os_model(taps, x, N, M=1, hist=None, pair=None, fft=None, ifft=None, resamp=False):
    """Overlap-save FIR (then keep every M-th output) on transforms of N points in complex64 -- the FP32 yardstick of the
    overlap-save families.  Output o is sum_k h[k] buf[o M + k], buf = [hist | x] with ntaps - 1 samples of history
    (FIR<T>) or ntaps (resamp: PolyphaseResampler<T> at interp 1).

    pair (real x only): None for complex data; "adjacent" rides segments (2p, 2p + 1) on one complex transform as re / im,
    "half" rides (p, p + ceil(nseg / 2)) -- the broken pairing.  fft / ifft: the transform pair (numpy's complex64 one by
    default; numpy >= 2 keeps complex64 in single precision)."""
    fft = fft or (lambda a: np.fft.fft(a, axis=-1))
    ifft = ifft or (lambda a: np.fft.ifft(a, axis=-1))
    h = np.asarray(taps, np.float32)
    nt = len(h)
    real = not np.iscomplexobj(x)
    x32 = np.asarray(x, np.float32 if real else np.complex64)
    buf = _hist(h, x32, hist, resamp)
    nfull = len(buf) - nt + 1                  # 'valid' outputs at step 1
    Lo = N - nt + 1                            # new outputs per segment
    nseg = -(-nfull // Lo)
    bufp = np.concatenate([buf, np.zeros(nseg * Lo + nt - 1 - len(buf), buf.dtype)])
    idx = np.arange(nseg)[:, None] * Lo + np.arange(N)[None, :]
    segs = bufp[idx]
    H = fft(np.concatenate([h, np.zeros(N - nt, np.float32)]).astype(np.complex64)[None, :])
    if real and pair is not None:
        half = (nseg + 1) // 2
        if pair == "adjacent":
            A = np.arange(0, nseg, 2)
            B = np.minimum(A + 1, nseg - 1)
        else:
            A = np.arange(half)
            B = np.where(A + half < nseg, A + half, A)
        z = (segs[A] + 1j * segs[B]).astype(np.complex64)
        yz = ifft(fft(z) * H)[:, nt - 1:].astype(np.complex64)
        ys = np.zeros((nseg, Lo), np.float32)
        ys[B] = yz.imag
        ys[A] = yz.real
    else:
        yc = ifft(fft(segs.astype(np.complex64)) * H)[:, nt - 1:].astype(np.complex64)
        ys = yc.real.astype(np.float32) if real else yc
    y = ys.reshape(-1)[:nfull]
    return y[::M][: len(x32) // M]


def os_yardsticks(taps, x, N, M=1, hist=None, resamp=False):
    """The two FP32 overlap-save yardsticks of a family of transform length N: numpy's complex64 FFT, and the textbook
    radix-2 transform with its twiddles rounded once to float32.  (On a pure-tone blocker numpy's transform errs ~80 x
    less than the radix-2 one -- less than the k-ordered direct chain -- while on white noise the two are within 2 x:
    the bound takes the larger of the two, region by region.)  Real data rides adjacent segment pairs."""
    pair = None if np.iscomplexobj(x) else "adjacent"
    r2 = dict(fft=fft_radix2, ifft=lambda a: fft_radix2(a, inverse=True))
    return [os_model(taps, x, N, M, hist=hist, pair=pair, resamp=resamp), os_model(taps, x, N, M, hist=hist, pair=pair, resamp=resamp, **r2)]


def direct_fma32(taps, x, M=1, hist=None, resamp=False):
    """The k-ordered FP32 dot product, product and sum rounded apart (numpy has no fused multiply-add): the honest
    baseline of the broken-model controls."""
    h = np.asarray(taps, np.float32)
    x32 = np.asarray(x, np.complex64 if np.iscomplexobj(x) else np.float32)
    buf = _hist(h, x32, hist, resamp)
    nout = len(x32) // M
    acc = np.zeros(nout, x32.dtype)
    for k in range(len(h)):
        acc = (acc + h[k] * buf[k: k + M * nout: M][:nout]).astype(x32.dtype)
    return acc


def padded_dot32(taps, x, M=1, pad=8):
    """Broken model (c): the dot product of direct_fma32 on taps zero-padded to a multiple of `pad` -- at the FRONT, so the
    zero taps multiply samples before the window (0 * NaN = NaN)."""
    h = np.asarray(taps, np.float32)
    npad = (-len(h)) % pad or pad
    hp = np.concatenate([np.zeros(npad, np.float32), h])
    x32 = np.asarray(x, np.complex64 if np.iscomplexobj(x) else np.float32)
    return direct_fma32(hp, x32, M, hist=np.zeros(len(hp) - 1, x32.dtype))


# ------------------------------------------------------------------------------------------------ region metric
def region_err(y, ref, mask):
    """(RMS, max) of |y - ref| over the outputs selected by mask."""
    d = np.abs(np.asarray(y).astype(np.complex128)[mask] - np.asarray(ref)[mask])
    if d.size == 0:
        return 0.0, 0.0
    return float(np.sqrt(np.mean(d * d))), float(d.max())


def region_check(y, yard, ref, regions, k=K, floor=FLOOR):
    """For each named region (boolean mask): the measured (rms, max) of y and of the yardstick against ref, the ratio, and
    whether y is inside k x yardstick + floor.  `yard` may be a list of yardsticks: the larger error of them, region by
    region and measure by measure.  Returns (ok, report)."""
    yards = yard if isinstance(yard, (list, tuple)) else [yard]
    ok, rep = True, {}
    for name, m in regions.items():
        g = region_err(y, ref, m)
        e = [region_err(v, ref, m) for v in yards]
        s = (max(v[0] for v in e), max(v[1] for v in e))
        good = bool(np.isfinite(g[0]) and g[0] <= k * s[0] + floor and g[1] <= k * s[1] + floor)
        rep[name] = dict(rms=g[0], max=g[1], yard_rms=s[0], yard_max=s[1], ratio=g[0] / s[0] if s[0] > 0 else float("inf") if g[0] > 0 else 0.0, ok=good)
        ok &= good
    return ok, rep


def loud_quiet_masks(first, last, loud_end, span, n_out):
    """Outputs whose window [first, last] lies in the loud part [0, loud_end) vs. at least `span` samples past it."""
    loud = last < loud_end
    quiet = first >= loud_end + span
    return {"loud": loud[:n_out], "quiet": quiet[:n_out]}


def poison_check(bad, first, last, t, span):
    """NaN / Inf locality: outputs whose window holds t must be bad; a bad output must lie within `span` samples of t.
    Returns (missing, stray): outputs that should be bad and are not, and bad outputs farther than span."""
    hold = (first <= t) & (t <= last)
    dist = np.maximum(0, np.maximum(first - t, t - last))
    missing = np.flatnonzero(hold & ~bad)
    stray = np.flatnonzero(bad & (dist > span))
    return missing, stray


# ------------------------------------------------------------------------------------------------ uniform channelizer
# The 64-channel polyphase + DFT channelizer (chan_uniform_kernel) restated from its documented operator (header of
# qdsp_amd/csrc/chan.hip).  Phases are the library's 64-bit fixed-point turns (2^64 = one turn), kept as wrapping uint64 /
# Python ints, so a phase is exact whatever the stream position; only the final conversion to an angle rounds (2^-53 turn).
_MASK64 = (1 << 64) - 1
CHAN_TOL_TURNS = 4e-7           # chan_uniform_plan: largest deviation of an increment from the grid d0 +- c / 64


def fx_of_inc(re, im):
    """Fixed-point turns per sample of a float (cos, sin) phase increment: the angle of the ROUNDED pair, as the library
    (turns_of / fx_of_turns, long double) and the oracle's exact-phase rotator (atan2 of the pair) take it."""
    ld = np.longdouble
    two_pi = ld(8) * np.arctan(ld(1))
    t = np.arctan2(ld(np.float32(im)), ld(np.float32(re))) / two_pi
    t = t - np.floor(t)
    hi = int(np.floor(np.ldexp(t, 32)))                      # (two exact 32-bit halves: no reliance on int(longdouble) being exact)
    lo = int(np.floor(np.ldexp(np.ldexp(t, 32) - ld(hi), 32)))
    return ((hi << 32) + lo) & _MASK64


def inc_of_turns(t):
    """The float32 (cos, sin) pair nearest to exp(j 2 pi t)."""
    a = 2.0 * np.pi * (float(t) % 1.0)
    return float(np.float32(np.cos(a))), float(np.float32(np.sin(a)))


def chan_uniform_plan(dphase):
    """chan_uniform_plan (chan_ops.hip): (inv, deltas) if the 64 fixed-point increments are channel 0's plus c * (+-2^58) to
    within 4e-7 turn -- inv: channel c at +c/64 turn per sample; deltas: signed deviations, delta_0 = 0 -- else None."""
    if len(dphase) != 64:
        return None
    tol = int(18446744073709551616.0 * CHAN_TOL_TURNS)
    for sign in (1, -1):
        dev = []
        for c in range(64):
            d = (int(dphase[c]) - (int(dphase[0]) + sign * c * (1 << 58))) & _MASK64
            dev.append(d - (1 << 64) if d >= (1 << 63) else d)
        if all(-tol <= d <= tol for d in dev):
            return sign > 0, dev
    return None


def _u64(v):
    """Python ints (any sign, any size) -> uint64 modulo 2^64; never through a numpy conversion of the list, which would go by float64."""
    return np.array([int(a) & _MASK64 for a in (v if isinstance(v, (list, tuple)) else [v])], dtype=np.uint64)


def fx_phasor(ph):
    """exp(j 2 pi ph / 2^64) of a uint64 array, complex128."""
    return np.exp(2j * np.pi * (np.asarray(ph, np.uint64).astype(np.float64) * 2.0 ** -64))


def _fx_outer(a, b):
    """a[:, None] * b[None, :] modulo 2^64."""
    with np.errstate(over="ignore"):
        return np.multiply.outer(np.asarray(a, np.uint64), np.asarray(b, np.uint64))


def _windows(buf, P, M, nout):
    """rows n' = buf[n' M : n' M + P] (buf long enough)."""
    return np.lib.stride_tricks.sliding_window_view(buf, P)[::M][:nout]


class ChanUniform64:
    """A 64-channel bank with the library's state -- per channel a fixed-point phase and increment, and the last P RAW input
    samples -- and two operators on it, both FP64, both for one call x (nout = len(x) // M outputs per channel, window n'
    starting at call-relative position j0 = n' M - P, i.e. restarting with every call like PolyphaseResampler):

      uniform(x): y_c[n'] = exp(j 2pi (j0 + kc) delta_c) sum_k h[k] x[j0 + k] exp(j 2pi (phi_c + (j0 + k)(dphi_c - delta_c)))
                  -- the operator chan.hip documents: the deviation delta_c of channel c's increment from the grid applied at the
                  window centre kc = (P - 1) // 2 instead of per tap;
      exact(x):   y_c[n'] = sum_k h[k] x[j0 + k] exp(j 2pi (phi_c + (j0 + k) dphi_c)) -- rotate, then filter (Splitter -> VFO).

    Broken-model switches (CPU controls only): kc_off moves the centre.  dphase overrides the increments (fixed point)."""

    def __init__(self, taps, phase_incs, M, dphase=None, kc_off=0):
        self.h = np.asarray(taps, np.float32).astype(np.float64)
        self.P, self.M = len(self.h), int(M)
        self.dphase = [int(d) & _MASK64 for d in dphase] if dphase is not None else [fx_of_inc(*pi) for pi in phase_incs]
        self.phase = [0] * len(self.dphase)
        self.hist = np.zeros(self.P, np.complex128)
        self.kc = (self.P - 1) // 2 + kc_off

    # -- state, as the C ABI moves it
    def reset(self):
        self.phase = [0] * len(self.dphase)
        self.hist[:] = 0

    def advance(self, n):
        self.phase = [(p + n * d) & _MASK64 for p, d in zip(self.phase, self.dphase)]

    def set_phase_inc(self, c, re, im):
        self.dphase[c] = fx_of_inc(re, im)

    def plan(self):
        return chan_uniform_plan(self.dphase)

    def _carry(self, buf, n):
        self.hist = buf[n: n + self.P].copy()
        self.advance(n)

    def _sum(self, x, base, extra):
        """sum_k h[k] buf[n' M + k] exp(j 2pi k base_c), times exp(j 2pi (phi_c + j0 dphi_c + extra_c)): (64, nout)."""
        n = len(x)
        nout = n // self.M
        buf = np.concatenate([self.hist, np.asarray(x).astype(np.complex128)])
        if nout:
            W = self.h[:, None] * fx_phasor(_fx_outer(np.arange(self.P, dtype=np.uint64), _u64(base)))
            S = _windows(buf, self.P, self.M, nout) @ W
            j0 = (np.arange(nout, dtype=np.int64) * self.M - self.P).view(np.uint64)
            with np.errstate(over="ignore"):
                rot = _fx_outer(j0, _u64(self.dphase)) + _u64(self.phase)[None, :] + _u64(extra)[None, :]
            y = (S * fx_phasor(rot)).T
        else:
            y = np.zeros((len(self.dphase), 0), np.complex128)
        self._carry(buf, n)
        return y

    def uniform(self, x):
        inv, delta = self.plan()
        return self._sum(x, [d - dl for d, dl in zip(self.dphase, delta)], [self.kc * dl for dl in delta])

    def exact(self, x):
        return self._sum(x, self.dphase, [0] * len(self.dphase))


def chan_uniform_ref64(taps, phase_incs, M, x, cuts, **kw):
    """The documented operator of the uniform channelizer over a stream cut into calls at `cuts`: (64, n_out) complex128."""
    r = ChanUniform64(taps, phase_incs, M, **kw)
    return np.concatenate([r.uniform(x[a:b]) for a, b in zip(cuts, cuts[1:])], axis=1)


def chan_uniform_windows(ntaps, M, cuts):
    """[first, last] stream positions of every output's P-tap window."""
    f = np.concatenate([a + np.arange((b - a) // M, dtype=np.int64) * M - ntaps for a, b in zip(cuts, cuts[1:])])
    return f, f + ntaps - 1


def chan_uniform_yard_call(st, xs, kc_off=0, mu_no_P=False, flip_inv=False):
    """One call of the kernel's own algorithm on the FP32 road from the state `st` (a ChanUniform64, left unchanged): the folded
    taps g[k] = h[k] exp(j 2pi k dphi_0) formed in FP64 and rounded to complex64 (chan_uniform_prepare), the 64 branch sums
    U[p] = sum_q g[64 q + p] x[j0 + 64 q + p] in complex64 in q order, a 64-point complex64 radix-2 DFT over mu = (p - P) mod 64
    (forward for the descending plan, conjugate twiddles for the ascending one) and ONE multiply by the FP64 phasor
    exp(j 2pi (phi_c + j0 dphi_c + kc delta_c +- c P / 64)) rounded to complex64.
    Broken models for the CPU controls: kc_off (window centre off by that many taps), mu_no_P (branches numbered mu = p while the
    +- c P / 64 correction stays), flip_inv (the other template sign: conjugated twiddles and sc flipped)."""
    P, M = st.P, st.M
    Q = -(-P // 64)
    xs = np.asarray(xs, np.complex64)
    nout = len(xs) // M
    if not nout:
        return np.zeros((64, 0), np.complex64)
    inv, delta = st.plan()
    if flip_inv:
        inv = not inv
    d0 = st.dphase[0]
    g = np.zeros(256, np.complex64)
    g[:P] = (st.h * fx_phasor(_fx_outer(np.arange(P, dtype=np.uint64), _u64(d0))[:, 0])).astype(np.complex64)
    buf = np.concatenate([st.hist.astype(np.complex64), xs, np.zeros(256, np.complex64)])       # (zeros behind the call)
    Xw = _windows(buf, 256, M, nout)
    U = np.zeros((nout, 64), np.complex64)
    for q in range(Q):
        U = (U + Xw[:, 64 * q: 64 * q + 64] * g[None, 64 * q: 64 * q + 64]).astype(np.complex64)
    T = np.zeros_like(U)
    p = np.arange(64)
    T[:, p if mu_no_P else (p - P) & 63] = U
    D = fft_radix2(T, inverse=True) * np.float32(64) if inv else fft_radix2(T)
    sc = [(c if inv else -c) for c in range(64)]
    inc = [(d0 + dl + (s << 58)) & _MASK64 for dl, s in zip(delta, sc)]                          # == dphase_c for the true sign
    j0 = (np.arange(nout, dtype=np.int64) * M - P).view(np.uint64)
    with np.errstate(over="ignore"):
        rot = _fx_outer(j0, _u64(inc)) + _u64(st.phase)[None, :] + _u64([(st.kc + kc_off) * dl + ((s * P) << 58) for dl, s in zip(delta, sc)])[None, :]
    return (D * fx_phasor(rot).astype(np.complex64)).astype(np.complex64).T


def chan_uniform_yardstick32(taps, phase_incs, M, x, cuts, dphase=None, **broken):
    """chan_uniform_yard_call over a stream cut into calls at `cuts`, state carried like chan_uniform_ref64: (64, n_out) complex64."""
    st = ChanUniform64(taps, phase_incs, M, dphase=dphase)
    out = []
    for a, b in zip(cuts, cuts[1:]):
        out.append(chan_uniform_yard_call(st, x[a:b], **broken))
        st._carry(np.concatenate([st.hist, np.asarray(x[a:b]).astype(np.complex128)]), b - a)
    return np.concatenate(out, axis=1)


def rotate_direct32(taps, dphase, phase, hist_raw, x, M):
    """Yardstick of one channel on a per-channel (rotate-then-filter) kernel: the FP64-phase NCO on [raw history | x] rounded to
    complex64, then the k-ordered FP32 chain of direct_fma32."""
    P = len(taps)
    buf = np.concatenate([np.asarray(hist_raw, np.complex128), np.asarray(x).astype(np.complex128)])
    j = (np.arange(len(buf), dtype=np.int64) - P).view(np.uint64)
    with np.errstate(over="ignore"):
        r = (buf * fx_phasor(j * np.uint64(int(dphase) & _MASK64) + np.uint64(int(phase) & _MASK64))).astype(np.complex64)
    return direct_fma32(taps, r[P:], M, hist=r[:P], resamp=True)


def chan_tones(n, dphase, loud_end, loud=17, weak=(16, 18, 49, 0, 63), weak_db=-100.0, off=0.0013, seed=0):
    """Check A's input for a 64-channel bank (FP64, not rounded): a 0 dBFS tone in channel `loud`'s band on [0, loud_end) and
    weak tones throughout in the bands of `weak`.  Channel c's band centre is the frequency its NCO brings to 0: -dphi_c."""
    ph = np.random.default_rng(seed).uniform(0, 2 * np.pi, 1 + len(weak))
    f = lambda c: -(int(dphase[c]) * 2.0 ** -64) + off                                               # noqa: E731
    x = gate(tone(n, f(loud), 1.0, phase=ph[0]), 0, loud_end)
    for i, c in enumerate(weak):
        x = x + tone(n, f(c), 10.0 ** (weak_db / 20.0), phase=ph[1 + i])
    return x


def chan_taps(ntaps, fc=0.4 / 64):
    """A Blackman-windowed sinc of any length >= 1 for the 64-channel bank (cutoff at 0.4 of the channel spacing), float32."""
    if ntaps < 3:
        return np.array([1.0, 0.5][:ntaps], np.float32)
    n = np.arange(ntaps, dtype=np.float64)
    h = 2 * fc * np.sinc(2 * fc * (n - (ntaps - 1) / 2.0))
    h *= 0.42 - 0.5 * np.cos(2 * np.pi * n / (ntaps - 1)) + 0.08 * np.cos(4 * np.pi * n / (ntaps - 1))
    return (h / h.sum()).astype(np.float32)


def chan_grid_incs(sign, detune=0.0, shift=0.0):
    """64 float (cos, sin) increments on the grid sign * (c - 31.5) / 64 + shift turns per sample; detune: channels 1..63 moved
    off it by +-detune turns, alternating (channel 0 defines the grid, so its own deviation is 0 by construction)."""
    return [inc_of_turns(sign * (c - 31.5) / 64 + shift + (0.0 if c == 0 else detune * (1 if c & 1 else -1))) for c in range(64)]
