"""The definition the MMClockRecovery tests hold the library to (include/qdsp_hip.h: symbol timing), restated in numpy.

mmse_taps()   the interpolator table's closed form, FP64
lib_taps()    the same, rounded as the library documents: what get_interp_taps returns
mm_ref()      the operator: float32 scalars, the eight products and their sum in FP64, one rounding to float32
mm_run()      the same recurrence with the dot product in another arithmetic (the orders VOLK's kernels use, in float32) or wholly
              in longdouble, with every decision it took recorded
"""
import math

import numpy as np

F = np.float32
STEPS, NTAPS, HALO = 128, 8, 7


def mmse_taps() -> np.ndarray:
    """Row m (mu = m / 128) solves R h = p, R[k][l] = sinc((k - l) / 2), p[k] = sinc((3 + mu - k) / 2); np.sinc is sin(pi x) / (pi x)."""
    k = np.arange(NTAPS, dtype=np.float64)
    R = np.sinc(0.5 * (k[:, None] - k[None, :]))
    mu = np.arange(STEPS + 1, dtype=np.float64) / STEPS
    P = np.sinc(0.5 * (3.0 + mu[None, :] - k[:, None]))
    return np.linalg.solve(R, P).T.copy()


def lib_taps() -> np.ndarray:
    """An entry below 1e-9 in magnitude is 0; every other is rounded to six significant decimal digits, then to float32."""
    h = mmse_taps()
    out = np.zeros(h.shape, dtype=np.float32)
    for i in range(h.shape[0]):
        for j in range(h.shape[1]):
            v = 0.0 if abs(h[i, j]) < 1e-9 else float(h[i, j])
            out[i, j] = np.float32(float("%.5e" % v))
    return out


def limits(omega, rel):
    omega, rel = F(omega), F(rel)
    return omega - (omega * rel), omega + (omega * rel)


def params(omega, gain_omega=0.01 * 0.01 / 4, mu_gain=0.01, rel_limit=0.005) -> dict:
    lo, hi = limits(omega, rel_limit)
    return {"omega": F(omega), "gain_omega": F(gain_omega), "mu_gain": F(mu_gain), "omega_min": lo, "omega_max": hi}


def param_ok(omega, gain_omega, mu_gain, rel_limit) -> bool:
    """The parameter rule."""
    v = [F(omega), F(gain_omega), F(mu_gain), F(rel_limit)]
    if not all(np.isfinite(v)) or not v[0] > 0 or not (0 <= v[3] < 1):
        return False
    lo, hi = limits(v[0], v[3])
    return bool(np.isfinite(hi) and lo - abs(v[2]) >= F(1) and hi + abs(v[2]) < F(2 ** 20))


def out_size(count: int, pars) -> int:
    lo = min(float(p["omega_min"] - abs(p["mu_gain"])) for p in pars)
    return -(-count // int(math.floor(lo))) if count > 0 else 0


def new_state(kind: int, par: dict) -> dict:
    zero = 0j if kind else 0.0
    return {"mu": F(0.5), "dyn": par["omega"], "next": 0, "det": [zero] * 4 if kind else [zero], "hist": [zero] * HALO}


def _dot(xs, ts, mode):
    """sum xs[k] ts[k], k = 0 .. 7, real xs"""
    if mode == "f64":            # the definition: exact products, added in tap order in FP64, rounded once
        acc = float(xs[0]) * float(ts[0])
        for k in range(1, NTAPS):
            acc = acc + float(xs[k]) * float(ts[k])
        return F(acc)
    if mode == "ld":
        acc = np.longdouble(0)
        for k in range(NTAPS):
            acc = acc + np.longdouble(xs[k]) * np.longdouble(ts[k])
        return acc
    pr = [F(xs[k]) * F(ts[k]) for k in range(NTAPS)]
    if mode == "seq32":
        acc = F(0)
        for v in pr:
            acc = acc + v
        return acc
    if mode == "quad32":         # four partial sums, then added
        a = [pr[j] + pr[j + 4] for j in range(4)]
        return (a[0] + a[1]) + (a[2] + a[3])
    if mode == "tree32":         # eight products, then a tree
        return ((pr[0] + pr[1]) + (pr[2] + pr[3])) + ((pr[4] + pr[5]) + (pr[6] + pr[7]))
    raise ValueError(mode)


def mm_run(x, kind: int, par: dict, state: dict = None, taps=None, mode: str = "f64"):
    """One call over the samples `x` of one row.  Returns (symbols, state, decisions); `state` is not modified.  decisions: per
    symbol (position in x, idx, step, slicer signs, error clamp, omega clamp)."""
    ld = mode == "ld"
    R = np.longdouble if ld else F
    taps = lib_taps() if taps is None else taps
    st = new_state(kind, par) if state is None else state
    mu, dyn, nxt, det = R(st["mu"]), R(st["dyn"]), int(st["next"]), list(st["det"])
    g_omega, g_mu, o_min, o_max = (R(par[k]) for k in ("gain_omega", "mu_gain", "omega_min", "omega_max"))
    xe = np.concatenate([np.asarray(st["hist"], dtype=np.complex64 if kind else np.float32), np.asarray(x, dtype=np.complex64 if kind else np.float32)])
    n = len(x)
    step1 = lambda v: R(1) if v > 0 else R(-1)
    out, dec = [], []
    bad = not (mu >= 0 and mu < 1)
    with np.errstate(all="ignore"):
        while not bad and nxt < n:
            idx = int(math.floor(float(mu * R(128)) + 0.5))          # roundf of a value >= 0
            idx = min(max(idx, 0), STEPS)
            w, t = xe[nxt:nxt + NTAPS], taps[idx]
            if kind:
                yr, yi = _dot(w.real, t, mode), _dot(w.imag, t, mode)
                out.append(complex(yr, yi))
                p1, p2, c1, c2 = det[0], det[1], det[2], det[3]          # (the old p0, p1, c0, c1)
                c0r, c0i = step1(yr), step1(yi)
                ur, ui, vr, vi = yr - R(p2.real), yi - R(p2.imag), c0r - R(c2.real), c0i - R(c2.imag)
                ea = (ur * R(c1.real)) - (ui * -R(c1.imag))
                eb = (vr * R(p1.real)) - (vi * -R(p1.imag))
                e = ea - eb
                det = [_C(yr, yi), p1, _C(c0r, c0i), c1]
                signs = (float(c0r), float(c0i))
            else:
                y = _dot(w, t, mode)
                out.append(y)
                last = R(det[0])
                e = (step1(last) * y) - (last * step1(y))
                det = [y]
                signs = (float(step1(y)),)
            ecl = 0
            if e > 1:
                e, ecl = R(1), 1
            if e < -1:
                e, ecl = R(-1), -1
            if e != e:
                bad = True
                break
            dyn = dyn + (g_omega * e)
            ocl = 0
            if dyn > o_max:
                dyn, ocl = o_max, 1
            elif dyn < o_min:
                dyn, ocl = o_min, -1
            mu = mu + dyn + (g_mu * e)
            step = np.floor(mu)
            dec.append((nxt, idx, int(step), signs, ecl, ocl))
            nxt += int(step)
            mu = mu - step
    hist = list(xe[len(xe) - HALO:])
    new = {"mu": R(np.nan) if bad else mu, "dyn": dyn, "next": 0 if bad else nxt - n, "det": det, "hist": hist}
    dt = (np.clongdouble if kind else np.longdouble) if ld else (np.complex64 if kind else np.float32)
    return np.asarray(out, dtype=dt), new, dec


class _C:
    """A complex value whose parts keep their type (numpy has no complex of two longdoubles that survives `complex()`)."""

    def __init__(self, re, im):
        self.real, self.imag = re, im


def mm_ref(x, kind: int, par: dict, state: dict = None, taps=None):
    """(symbols, state) of one call over one row: the definition."""
    y, st, _ = mm_run(x, kind, par, state, taps, "f64")
    return y, st


def signal(kind: int, sps: float, nsym: int, seed: int, offset: float = 0.0, noise: float = 0.02) -> np.ndarray:
    """QPSK (kind 1) or +-1 (kind 0) symbols through a raised-cosine pulse (roll-off 0.35, cut at +-6 symbols) at `sps` samples per
    symbol, delayed by `offset` samples, plus noise."""
    rng = np.random.default_rng(seed)
    n = int(math.ceil(nsym * sps))
    if kind:
        sym = ((rng.integers(0, 2, nsym) * 2 - 1) + 1j * (rng.integers(0, 2, nsym) * 2 - 1)).astype(np.complex128)
    else:
        sym = (rng.integers(0, 2, nsym) * 2 - 1).astype(np.float64)
    pos = (np.arange(n, dtype=np.float64) - offset) / sps - 0.5          # in symbols: symbol k sits at pos == k
    k0 = np.rint(pos).astype(np.int64)
    x = np.zeros(n, dtype=sym.dtype)
    for j in range(-6, 7):
        k = k0 + j
        ok = (k >= 0) & (k < nsym)
        u = pos - k
        den = 1 - (0.7 * u) ** 2
        pulse = np.sinc(u) * np.cos(0.35 * np.pi * u) / np.where(np.abs(den) < 1e-9, 1.0, den)
        x += np.where(ok, sym[np.clip(k, 0, nsym - 1)] * pulse, 0)
    if kind:
        x = x + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        return x.astype(np.complex64)
    return (x + noise * rng.standard_normal(n)).astype(np.float32)
