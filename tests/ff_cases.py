"""Streams for the tests of the feed-forward ARGOS bits (a plain module beside argos_best_cases.py, no fixtures here), shared
by tests/test_ff.py (the host restatement against a Python model written from the rule's text) and tests/test_gpu_ff.py (the kernels
against the host restatement): small streams around every length at which the number of half-bits changes, zeros, NaN, Inf, the
metric's clamp, crafted ties; whole bursts with a bit-rate error, built here; the real recording both ways round."""
import functools
import math
from fractions import Fraction

import numpy as np

import real_captures as rc
from argos_msg_cases import CODES, SYNC

F32 = np.float32


# ---------------------------------------------------------------- the rule, from its text
def round_f32(q: Fraction) -> np.float32:
    """a rational number rounded to the nearest float32, ties to even (never called with 0)"""
    s, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    m = q / ulp
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    v = n * ulp
    return F32(s * float(v)) if v < Fraction(2) ** 128 else F32(s * math.inf)


def fmaf(a, b, c) -> np.float32:
    """a b + c with one rounding, a, b, c float32"""
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))
    q = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if q == 0:
        x_neg = bool(np.signbit(a)) != bool(np.signbit(b))
        exact_zero_terms = (a == 0 or b == 0) and c == 0
        return F32(-0.0) if exact_zero_terms and x_neg and np.signbit(c) else F32(0.0)
    return round_f32(q)


def chain_sum(seg: np.ndarray) -> np.float32:
    """the float32 addition chain from +0 in ascending index"""
    with np.errstate(all="ignore"):
        return np.cumsum(np.concatenate([np.zeros(1, F32), seg.astype(F32)]), dtype=F32)[-1]


def period(H: int, r: int, ppm: float) -> int:
    return int(np.rint(np.float64(H) * 65536.0 * (1.0 + r * ppm * 1e-6)))


def bound(k: int, P: int) -> int:
    return (k * P + 32768) >> 16


def halves(L: int, tau: int, P: int) -> int:
    k = 0
    while tau + bound(k + 2, P) <= L:
        k += 2
    return k


def quant(d) -> int:
    if not np.isfinite(d):
        return 0
    a = abs(float(d))
    return 1 << 52 if a >= 2.0 ** 20 else int(Fraction(a) * 2 ** 32)


def model(v: np.ndarray, fs: int, R: int, ppm: float = 625.0):
    """(tau, r, P, M, bits, soft, index, the whole table M[(r, tau)]) of the mixed stream v, float32[n, 2]"""
    H = fs // 800
    v = np.asarray(v, dtype=F32).reshape(-1, 2)[: 2 * fs]
    L = len(v)

    def d_of(tau, P, m):
        b = [tau + bound(2 * m + j, P) for j in range(3)]
        ar, ai = chain_sum(v[b[0]:b[1], 0]), chain_sum(v[b[0]:b[1], 1])
        br, bi = chain_sum(v[b[1]:b[2], 0]), chain_sum(v[b[1]:b[2], 1])
        with np.errstate(all="ignore"):
            p = F32(ar * bi)
        return fmaf(ai, br, -p)

    table, best = {}, None
    for r in range(-R, R + 1):
        P = period(H, r, ppm)
        for tau in range(2 * H):
            M = sum(quant(d_of(tau, P, m)) for m in range(halves(L, tau, P) // 2))
            table[(r, tau)] = M
            key = (-M, abs(r), r, tau)
            if best is None or key < best:
                best = key
    _, _, r, tau = best
    P = period(H, r, ppm)
    soft = np.array([d_of(tau, P, m) for m in range(halves(L, tau, P) // 2)], dtype=F32)
    soft.view(np.uint32)[np.isnan(soft)] = 0x7FC00000                     # a NaN is stored as the quiet NaN 0x7fc00000
    bits = np.where(soft > 0, ord("1"), ord("0")).astype(np.uint8)
    index = np.array([tau + bound(2 * m + 2, P) for m in range(len(soft))], dtype=np.int64)
    return tau, r, P, table[(r, tau)], bits, soft, index, table


# ---------------------------------------------------------------- small streams
def small_lengths(H: int):
    """0, 1, around one bit, two bits, and the lengths at which the last offset holds a bit less than the first"""
    return [0, 1, 2 * H - 1, 2 * H, 2 * H + 1, 4 * H, 4 * H + 2 * H - 2, 4 * H + 2 * H - 1, 6 * H - 1, 6 * H + 3]


def small_streams(H: int):
    """(name, float32[n, 2]) for one H: noise of every length of small_lengths, zeros, a NaN and an Inf sample, amplitude 1e6 (the
    clamp), and sparse streams of powers of two whose sums are exact and whose metrics tie"""
    rng = np.random.default_rng(1000 + H)
    out = []
    for n in small_lengths(H):
        out.append((f"noise-n{n}", rng.standard_normal((n, 2)).astype(F32)))
    n = 6 * H + 3
    out.append(("zeros", np.zeros((n, 2), F32)))
    for name, bad in (("nan", np.nan), ("inf", np.inf), ("minus-inf", -np.inf)):
        y = rng.standard_normal((n, 2)).astype(F32)
        y[2 * H + 1, 1] = bad
        out.append((name, y))
    out.append(("clamp", (rng.standard_normal((n, 2)) * 1e6).astype(F32)))
    out.append(("huge", (rng.standard_normal((n, 2)) * 1e30).astype(F32)))
    out.append(("real-only", np.stack([rng.standard_normal(n), np.zeros(n)], axis=1).astype(F32)))
    for k in range(4):
        # a few samples of +-2^j: every half-bit sum is exact, many hypotheses share the largest metric
        y = np.zeros((12 * H + k, 2), F32)
        at = rng.choice(len(y), size=6, replace=False)
        y[at, rng.integers(0, 2, size=6)] = (2.0 ** rng.integers(-3, 4, size=6)) * rng.choice([-1.0, 1.0], size=6)
        out.append((f"tie{k}", y))
    return out


# ---------------------------------------------------------------- whole bursts
BURST_FS = 16000
BURST_ID, BURST_BLOCKS = 0x2D5A7, 8
RATE_ERRORS = (0.0, 0.004, 0.0125, -0.0125)


def burst_data() -> bytes:
    return bytes((37 * i + 11) & 0xFF for i in range(4 * BURST_BLOCKS))


def burst_bits() -> str:
    body = format(BURST_ID, "020b") + "".join(format(b, "08b") for b in burst_data())
    return "1" * 15 + SYNC + CODES[BURST_BLOCKS - 1] + body


@functools.lru_cache(maxsize=None)
def burst(rate_error: float, fs: int = BURST_FS, residual_hz: float = 37.3, seed: int = 5) -> np.ndarray:
    """0.16 s of carrier, then burst_bits() as +-1.1 rad Manchester at 400 (1 + rate_error) bit/s, amplitude 0.25 over noise of sigma
    0.05 per component, 0.03 s of noise behind it: float32[n, 2], read only"""
    bits = burst_bits()
    half = 1.0 / (800.0 * (1.0 + rate_error))
    n = int(round((0.16 + len(bits) * 2 * half + 0.03) * fs))
    t = np.arange(n) / fs
    k = np.floor((t - 0.16) / half).astype(np.int64)
    on = (k >= 0) & (k < 2 * len(bits))
    b = np.array([int(c) for c in bits])[np.clip(k // 2, 0, len(bits) - 1)]
    phase = np.where(on, 1.1 * np.where((k & 1) == 0, 1.0, -1.0) * np.where(b == 1, 1.0, -1.0), 0.0)
    live = t < 0.16 + len(bits) * 2 * half
    rng = np.random.default_rng(seed)
    z = 0.25 * live * np.exp(1j * (2 * np.pi * residual_hz * t + 0.7 + phase)) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    y = np.stack([z.real, z.imag], axis=1).astype(F32)
    y.setflags(write=False)
    return y


def decoded(pdt, bits: np.ndarray, rule: int = 0):
    """[(blocks, id, data, inverted)] of the complete messages in a string of bits"""
    m = pdt.host_argos_messages(bits.tobytes(), rule=rule)
    return [(int(r["blocks"]), int(r["id"]), bytes(r["data"][: 4 * r["blocks"]]), int(r["inverted"])) for r in m if r["complete"]]


def burst_decodes(pdt, bits: np.ndarray) -> bool:
    got = decoded(pdt, bits)
    return len(got) == 1 and got[0][:3] == (BURST_BLOCKS, BURST_ID, burst_data())


# ---------------------------------------------------------------- the real recording
@functools.lru_cache(maxsize=None)
def real(mirrored: bool) -> np.ndarray:
    """tests/golden/argos_packet.wav, uncut, as float32 (value / 32768); mirrored: Q negated"""
    rate, iq = rc.capture("packet")
    assert rate == 32000
    y = rc.as_float(iq).copy()
    if mirrored:
        y[:, 1] = -y[:, 1]
    y.setflags(write=False)
    return y


REAL_MESSAGE = (1, 0x01D81, bytes([0x00, 0x55, 0xAA, 0xFF]))


def same_bits(a, b) -> bool:
    """two FfBits, byte for byte: record, characters, soft bit patterns, sample indices"""
    return (a.sync.tobytes() == b.sync.tobytes() and a.bits.tobytes() == b.bits.tobytes() and a.soft.tobytes() == b.soft.tobytes()
            and a.index.tobytes() == b.index.tobytes())
