"""The contract of the audio input stage (include/lsprs.h) restated in numpy: a float64 model, and the float32 restatement whose error
against that model sizes the GPU test's bound.  Nothing here reads the library.

    g = gcd(Fi, 16000), L = 16000 / g, M = Fi / g, s = min(1, 16000 / Fi), Z = 64, beta = 14.769656459379492, rho = 0.9475937167399596
    h(u) = s rho sinc(s rho u) I0(beta sqrt(1 - (s u / Z)^2)) / I0(beta)  for |s u| < Z, else 0;  R = ceil(Z / s)
    y[j] = sum_{i = 0 .. 2R} h(p_j / L + R - i) x[c_j - R + i],  c_j = (j M) div L, p_j = (j M) mod L,  x = 0 outside [0, N)
    a stream of N samples has ceil(N L / M) outputs
"""
import math

import numpy as np

OUT_RATE = 16000
Z = 64
BETA = 14.769656459379492
RHO = 0.9475937167399596
RATES = (48000, 44100, 32000, 24000, 22050, 8000)


def ratio(rate):
    g = math.gcd(int(rate), OUT_RATE)
    L, M = OUT_RATE // g, int(rate) // g
    s = min(1.0, L / M)
    R = math.ceil(Z * M / L) if M > L else Z
    assert R == math.ceil(Z / s) or abs(Z / s - round(Z / s)) < 1e-9
    return L, M, R


def h(num, L, M):
    """h at u = num / L input samples (num: integer array), float64"""
    num = np.asarray(num, np.int64)
    s = min(1.0, L / M)
    u = num.astype(np.float64) / L
    inside = np.abs(num) < Z * max(L, M)                                           # |s u| < Z, decided on the integers
    w = np.where(inside, s * u / Z, 0.0)
    win = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - w * w))) / np.i0(BETA)
    return np.where(inside, s * RHO * np.sinc(s * RHO * u) * win, 0.0)


def table(rate):
    """coef[p][i] = h(p / L + R - i), float64 [L][2R + 1]"""
    L, M, R = ratio(rate)
    p, i = np.arange(L)[:, None], np.arange(2 * R + 1)[None, :]
    return h(p + (R - i) * L, L, M)


def n_out(rate, n):
    L, M, _ = ratio(rate)
    return -(-n * L // M)


def final_outputs(rate, n, finished):
    """the finality rule: output j is final when c_j + R <= n - 1, or when the stream has finished"""
    L, M, R = ratio(rate)
    if finished:
        return n_out(rate, n)
    j = np.arange(n_out(rate, n), dtype=np.int64)
    return int(((j * M) // L + R <= n - 1).sum())                                  # brute force: every tap of output j is present


def _windows(x, rate, dtype):
    L, M, R = ratio(rate)
    n = len(x)
    j = np.arange(n_out(rate, n), dtype=np.int64)
    c, p = (j * M) // L, (j * M) % L
    xp = np.concatenate([np.zeros(R, dtype), np.asarray(x, dtype), np.zeros(R + M // L + 2, dtype)])
    return xp, c, p, R                                                             # x[c - R + i] == xp[c + i]


def resample64(x, rate):
    """the float64 model: double taps, double sums"""
    xp, c, p, R = _windows(x, rate, np.float64)
    t = table(rate)
    y = np.zeros(len(c))
    for i in range(2 * R + 1):
        y += t[p, i] * xp[c + i]
    return y


def resample32_sequential(x, rate):
    """the contract's arithmetic without fmaf: float32 taps, one float32 accumulator per output, ascending taps, the product and the sum
    rounded separately"""
    xp, c, p, R = _windows(x, rate, np.float32)
    t = table(rate).astype(np.float32)
    y = np.zeros(len(c), np.float32)
    for i in range(2 * R + 1):
        y = (y + (t[p, i] * xp[c + i]).astype(np.float32)).astype(np.float32)
    return y


def to_mono_f32(raw):
    """the stage's conversion: int16 / 32768.0f, two channels averaged as (a + b) * 0.5f after conversion"""
    a = np.asarray(raw)
    a = (a.astype(np.float32) / np.float32(32768.0)) if a.dtype == np.int16 else a.astype(np.float32)
    if a.ndim == 2:
        a = ((a[:, 0] + a[:, 1]).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    return a
