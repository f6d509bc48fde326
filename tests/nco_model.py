"""The numpy model of gateware/bbb/nco.py (n = 24, m = 10, p = 16) that the NCO tests compare against: the module's registers
clocked one sample at a time, and the closed form the kernels use.  Inputs are a constant (int) or an array per sample; array
values are taken modulo their widths (fm: low 24 bits, pm: low 10 bits)."""
import numpy as np

MASK = (1 << 24) - 1


def rom():
    """nco.py:30-31: np.round(np.sin(np.linspace(0, 2 pi, 2^m)) * (2^(p-1) - 1)), kept signed."""
    return np.round(np.sin(np.linspace(0, 2 * np.pi, 1024)) * 32767).astype(np.int64)


ROM = rom()


def _at(v, t):
    return int(v[t]) if isinstance(v, np.ndarray) else int(v)


def clock(n, fcw, fm=0, am=0xFFFF, pm=0, state=(0, 0, 0, 0)):
    """The registers, one clock per sample: x(t) = y >> 16; adr = pa[14:24] + pm; pa += fcw + fm; q <= rom[adr]; w <= q;
    y <= am * w.  Returns (x int16[n], state after)."""
    pa, q, w, y = (int(s) for s in state)
    x = np.empty(n, dtype=np.int16)
    for t in range(n):
        x[t] = y >> 16
        adr = ((pa >> 14) + _at(pm, t)) & 1023
        pa, q, w, y = (pa + fcw + _at(fm, t)) & MASK, int(ROM[adr]), q, _at(am, t) * w
    return x, (pa, q, w, y)


def closed(n, fcw, fm=0, am=0xFFFF, pm=0, state=(0, 0, 0, 0)):
    """x(0) = y0 >> 16, x(k) = (am(k - 1) * R(k - 3)) >> 16 with R(j) = rom[((pa(j) >> 14) + pm(j)) mod 1024],
    R(-1) = q0, R(-2) = w0 and pa(j) = pa0 + sum_{s<j} (fcw + fm(s)) mod 2^24.  Vectorised; returns (x, state after)."""
    pa0, q0, w0, y0 = (int(s) for s in state)
    if isinstance(fm, np.ndarray):
        inc = (fcw + (fm[:n].astype(np.int64) & MASK)) & MASK
        csum = np.cumsum(inc)
        pa = (pa0 + np.concatenate(([0], csum[:-1]))) & MASK
        pa_end = (pa0 + int(csum[-1])) & MASK if n else pa0
    else:
        inc = (fcw + fm) & MASK
        pa = (pa0 + np.arange(n, dtype=np.int64) * inc) & MASK
        pa_end = (pa0 + n * inc) & MASK
    pmv = pm[:n].astype(np.int64) if isinstance(pm, np.ndarray) else pm
    r = np.concatenate(([0, w0, q0], ROM[((pa >> 14) + pmv) & 1023]))     # r[j + 3] = R(j)
    amv = am[:n].astype(np.int64) if isinstance(am, np.ndarray) else np.full(n, am, dtype=np.int64)
    x = np.empty(n, dtype=np.int16)
    if n:
        x[0] = y0 >> 16
        x[1:] = (amv[:n - 1] * r[1:n]) >> 16
        return x, (pa_end, int(r[n + 2]), int(r[n + 1]), int(amv[n - 1] * r[n]))
    return x, (pa0, q0, w0, y0)


def closed_at(t0, n, fcw, fm=0, am=0xFFFF, pm=0):
    """Constant inputs: x(t0 .. t0 + n - 1) from reset, for any t0 (pa(j) depends on j mod 2^24 only)."""
    inc = (fcw + fm) & MASK
    j = (t0 % (1 << 24)) + np.arange(n, dtype=np.int64) - 3           # adr(t - 3)
    r = ROM[((((j * inc) & MASK) >> 14) + pm) & 1023]
    r[np.arange(n) + t0 < 3] = 0
    return ((am * r) >> 16).astype(np.int16)
