"""The loudness contract of include/blissgpu.h restated in numpy and plain Python floats: the tables by their
formulas, the segmented K-weighting filter vectorised over segments, the true-peak interpolator, the blocks, the gates and the
range.  Shared by tests/test_loudness_host.py and tests/test_gpu_loudness.py; nothing here calls the code under test."""
import math
import os
import re

import numpy as np

from conftest import ROOT

ABS_GATE = 1.1724653045822981e-07


def header_constants():
    """(S, W): BLISSGPU_LOUDNESS_SEGMENT and _WARMUP as the header states them"""
    text = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
                 for name in ("BLISSGPU_LOUDNESS_SEGMENT", "BLISSGPU_LOUDNESS_WARMUP"))


def hop(rate):
    return (rate + 5) // 10


def kweighting(rate):
    """the ten coefficients by the issue's formulas, in Python floats"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
          (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return np.array(s1 + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def peak_factor(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def peak_filter(F):
    i = np.arange(49)
    return np.sinc((i - 24) / F) * (0.5 * (1.0 - np.cos(2.0 * np.pi * i / 48.0)))


def widen(a):
    """decoder output -> f64 [frames, channels], exactly"""
    a = np.asarray(a)
    a = a.reshape(a.shape[0], -1)
    if a.dtype == np.int16:
        return a.astype(np.float64) / 32768.0
    if a.dtype == np.int32:
        return a.astype(np.float64) / 2147483648.0
    return a.astype(np.float32).astype(np.float64)


def segment_energies(songs, S, W, coefs=None):
    """The segmented contract for a list of (x f64 [frames, channels], rate): every (song, channel, segment) is one row of one
    numpy loop over max (W + S) H steps, whatever the songs' lengths.  coefs: one table of ten per song (default: the formula).
    -> a list of z [channels, n_sub]"""
    rows = []   # (song, channel, first frame, frames, first sub-block kept, sub-blocks walked)
    out = []
    for s, (x, rate) in enumerate(songs):
        H = hop(rate)
        n_sub = x.shape[0] // H
        out.append(np.zeros((x.shape[1], n_sub)))
        for c in range(x.shape[1]):
            for g in range((n_sub + S - 1) // S):
                u0, u1 = max(0, g * S - W), min((g + 1) * S, n_sub)
                rows.append((s, c, u0 * H, (u1 - u0) * H, g * S - u0, u1 - u0))
    if not rows:
        return out
    R, steps = len(rows), max(r[3] for r in rows)
    X = np.zeros((steps, R))
    for k, (s, c, f0, n, _, _) in enumerate(rows):
        X[:n, k] = songs[s][0][f0:f0 + n, c]
    co = np.array([(kweighting(songs[r[0]][1]) if coefs is None else np.asarray(coefs[r[0]], np.float64)) for r in rows]).T.copy()
    b10, b11, b12, a11, a12, b20, b21, b22, a21, a22 = co
    Hs = np.array([hop(songs[r[0]][1]) for r in rows])
    s11, s12, s21, s22, acc = (np.zeros(R) for _ in range(5))
    cnt = np.zeros(R, np.int64)
    sub = np.zeros(R, np.int64)
    E = np.zeros((R, S + W))
    ends = np.zeros(steps, bool)   # the steps at which some row finishes a sub-block
    for H in set(Hs.tolist()):
        ends[H - 1::H] = True
    lane = np.arange(R)
    for t in range(steps):
        x = X[t]
        y1 = b10 * x + s11
        s11 = (b11 * x - a11 * y1) + s12
        s12 = b12 * x - a12 * y1
        y2 = b20 * y1 + s21
        s21 = (b21 * y1 - a21 * y2) + s22
        s22 = b22 * y1 - a22 * y2
        acc = acc + y2 * y2
        cnt += 1
        if ends[t]:
            done = cnt == Hs
            if done.any():
                d = lane[done & (sub < S + W)]
                E[d, sub[d]] = acc[d]
                sub[done] += 1
                acc[done] = 0.0
                cnt[done] = 0
    for k, (s, c, f0, n, skip, walked) in enumerate(rows):
        u_first = f0 // hop(songs[s][1]) + skip
        out[s][c, u_first:u_first + walked - skip] = E[k, skip:walked]
    return out


def peaks(x, rate, h=None):
    """(sample peak, true peak) of x f64 [frames, channels] by the contract: every phase's taps in ascending order, from 0.0"""
    F = peak_factor(rate)
    h = peak_filter(F) if h is None else np.asarray(h, np.float64)
    n, reach = x.shape[0], 24 // F
    tp = 0.0
    for c in range(x.shape[1]):
        pad = np.zeros(n + 48)
        pad[24:24 + n] = x[:, c]
        for p in range(F):
            acc = np.zeros(n)
            for j, i in enumerate(range(p, 49, F)):
                acc = acc + h[i] * pad[24 + reach - j:24 + reach - j + n]
            tp = max(tp, float(np.abs(acc).max())) if n else tp
    return (float(np.abs(x).max()) if x.size else 0.0), tp


def blocks(z, H):
    """z [channels, n_sub] -> (P, ST) as lists of Python floats, every sum in the contract's order"""
    z = np.asarray(z, np.float64)
    z = z.reshape(z.shape[0] if z.ndim == 2 else 1, -1).tolist()
    n_sub = len(z[0])
    P, ST = [], []
    for j in range(n_sub - 3):
        total = 0.0
        for zc in z:
            total = total + (((zc[j] + zc[j + 1]) + zc[j + 2]) + zc[j + 3])
        P.append(total / float(4 * H))
    for j in range(n_sub - 29):
        total = 0.0
        for zc in z:
            for u in range(j, j + 30):
                total = total + zc[u]
        ST.append(total / float(30 * H))
    return P, ST


def _mean(values):
    total = 0.0
    for v in values:
        total = total + v
    return total / float(len(values))


def lufs_of(power):
    return -0.691 + 10.0 * math.log10(power) if power > 0.0 else -math.inf


def gate(P):
    """(power, lufs) of BS.1770-4's two gates"""
    above = [p for p in P if p > ABS_GATE]
    if not above:
        return 0.0, -math.inf
    gamma = _mean(above) * 0.1
    kept = [p for p in above if p > gamma]
    power = _mean(kept) if kept else 0.0
    return power, lufs_of(power)


def loudness_range(ST):
    """(range_lu, lo, hi) of EBU Tech 3342"""
    above = [p for p in ST if p > ABS_GATE]
    if not above:
        return 0.0, 0.0, 0.0
    rel = _mean(above) * 0.01
    kept = sorted(p for p in above if p > rel)
    if not kept:
        return 0.0, 0.0, 0.0
    n = len(kept)
    lo, hi = kept[int((n - 1) * 0.10 + 0.5)], kept[int((n - 1) * 0.95 + 0.5)]
    return 10.0 * math.log10(hi / lo), lo, hi


def sine(rate, freq, levels_dbfs, seconds, channels=2, phase=0.0):
    """a sine whose peak level steps through levels_dbfs, each for its number of seconds; f64 [frames, channels], in phase"""
    amps = np.concatenate([np.full(int(round(sec * rate)), 10.0 ** (db / 20.0)) for db, sec in zip(levels_dbfs, seconds)])
    x = amps * np.sin(2.0 * np.pi * freq * np.arange(amps.size) / rate + phase)
    return np.repeat(x[:, None], channels, axis=1)


# EBU Tech 3341 cases 1 - 5 (1 kHz, stereo, in phase): (levels, seconds, expected LUFS, tolerance)
TECH_3341 = [
    ([-23.0], [20.0], -23.0, 0.1),
    ([-33.0], [20.0], -33.0, 0.1),
    ([-36.0, -23.0, -36.0], [10.0, 60.0, 10.0], -23.0, 0.1),
    ([-72.0, -36.0, -23.0, -36.0, -72.0], [10.0, 10.0, 60.0, 10.0, 10.0], -23.0, 0.1),
    ([-26.0, -20.0, -26.0], [20.0, 20.1, 20.0], -23.0, 0.1),
]
# EBU Tech 3342 cases 1 - 4 (20 s a step): (levels, expected LRA, tolerance)
TECH_3342 = [
    ([-20.0, -30.0], 10.0, 1.0),
    ([-20.0, -15.0], 5.0, 1.0),
    ([-40.0, -20.0], 20.0, 1.0),
    ([-50.0, -35.0, -20.0, -35.0, -50.0], 15.0, 1.0),
]
