"""Streams for the tests of the feed-forward POES bits (a plain module beside ff_cases.py, no fixtures here), shared by
tests/test_ffp.py (the host restatement against a Python model written from the rule's text) and tests/test_gpu_ffp.py (the kernels
against the host restatement): small streams with a carrier and Manchester PM of known bits at every rate the rule's cases name,
every stream length at which something changes, a drifting clock, a block of zeros, Inf and NaN, tone-segment seams."""
import functools

import numpy as np

from ff_cases import F32, fmaf, quant

RATES = (49920, 50000, 250000, 1064960)
SMALL = dict(block_bits=64, clock_steps=8, ref_bits=4, smooth_blocks=1)       # what most cases run under: the model is plain Python


# ---------------------------------------------------------------- the rule, from its text
def t_k(k: int, fs: int) -> int:
    return (k * fs * 65536) // 16640


def offset(f: int, fs: int, T: int) -> int:
    return (f * 2 * fs * 65536) // (16640 * T)                                # (Python's // rounds towards minus infinity)


def block_len(B: int, fs: int) -> int:
    return (2 * B * fs + 8320) // 16640


def first_bit(x: int, off: int, fs: int) -> int:
    """the smallest m >= 0 with t_2m + off >= x"""
    m = max(0, (x - off) * 16640 // (2 * fs * 65536) - 2)
    while t_k(2 * m, fs) + off < x:
        m += 1
    return m


def last_bit(n: int, off: int, fs: int) -> int:
    """the largest m with t_2m+2 + off <= n 65536, -1 when there is none"""
    m = ((n << 16) - off) * 16640 // (2 * fs * 65536) + 2
    while m >= 0 and t_k(2 * m + 2, fs) + off > (n << 16):
        m -= 1
    return max(m, -1)


def interval_sum(v: np.ndarray, a: int, b: int):
    """the fma chain over the Q16 interval [a, b): (re, im)"""
    i0, i1 = a >> 16, (b - 1) >> 16
    out = []
    for comp in (0, 1):
        acc = F32(0.0)
        i = i0
        while i <= i1:
            lo, hi = (a if i == i0 else i << 16), (b if i == i1 else (i + 1) << 16)
            if hi - lo == 65536:
                # a run of whole samples: fmaf(v, 1, s) is the float addition
                j = i1 if (b - (i1 << 16)) == 65536 else i1 - 1
                with np.errstate(all="ignore"):
                    acc = np.cumsum(np.concatenate([np.array([acc], F32), v[i:j + 1, comp]]), dtype=F32)[-1]
                i = j + 1
            else:
                acc = fmaf(v[i, comp], F32((hi - lo) / 65536.0), acc)
                i += 1
        out.append(acc)
    return out


def cross(er, ei, rr, ri) -> np.float32:
    with np.errstate(all="ignore"):
        p = F32(F32(er) * F32(ri))
    return fmaf(ei, rr, -p)


def model(v: np.ndarray, fs: int, block_bits=None, clock_steps=None, ref_bits=None, smooth_blocks=None, residual_hz=None):
    """the rule on the mixed stream v, float32[n, 2]: dict(bits, soft, index, blocks = [(tau, phi, first_bit, count, metric)])"""
    B, T = block_bits or 208, clock_steps or 32
    W = 16 if ref_bits is None else ref_bits
    J = 4 if smooth_blocks is None else smooth_blocks
    v = np.asarray(v, dtype=F32).reshape(-1, 2)
    n = len(v)
    L = block_len(B, fs)
    nb = (n + L - 1) // L

    @functools.lru_cache(maxsize=None)
    def pairs(off):
        """(lo, hi, c, e) of the bits that exist under `off`"""
        lo, hi = first_bit(0, off, fs), last_bit(n, off, fs)
        c, e = [], []
        for m in range(lo, hi + 1):
            a0, a1, a2 = (t_k(2 * m + j, fs) + off for j in range(3))
            h0, h1 = interval_sum(v, a0, a1), interval_sum(v, a1, a2)
            with np.errstate(all="ignore"):
                c.append((F32(h0[0] + h1[0]), F32(h0[1] + h1[1])))
                e.append((F32(h0[0] - h1[0]), F32(h0[1] - h1[1])))
        return lo, hi, c, e

    def soft_of(off, m):
        lo, hi, c, e = pairs(off)
        rr, ri = F32(0.0), F32(0.0)
        with np.errstate(all="ignore"):
            for k in range(max(lo, m - W), min(hi, m + W) + 1):
                rr, ri = F32(rr + c[k - lo][0]), F32(ri + c[k - lo][1])
        return cross(e[m - lo][0], e[m - lo][1], rr, ri)

    M = np.zeros((nb, T), dtype=object)
    for tau in range(T):
        off = offset(tau, fs, T)
        lo, hi, _, _ = pairs(off)
        for m in range(lo, hi + 1):
            M[((t_k(2 * m, fs) + off) >> 16) // L, tau] += quant(soft_of(off, m))
    taus, metrics = [], []
    for b in range(nb):
        Ms = [sum(M[k, tau] for k in range(max(0, b - J), min(nb - 1, b + J) + 1)) for tau in range(T)]
        taus.append(min(t for t in range(T) if Ms[t] == max(Ms)))            # ties to the smaller tau
        metrics.append(int(max(Ms)))
    phis = []
    for b in range(nb):
        if b == 0:
            phis.append(taus[0])
            continue
        d = (taus[b] - taus[b - 1]) % T
        phis.append(phis[-1] + (d - T if 2 * d > T else d))
    bits, soft, index, blocks = [], [], [], []
    for b in range(nb):
        off = offset(phis[b], fs, T)
        lo = first_bit((b * L) << 16, off, fs)
        hi = last_bit(n, off, fs) + 1
        if b + 1 < nb:
            hi = min(hi, first_bit(((b + 1) * L) << 16, offset(phis[b + 1], fs, T), fs))
        blocks.append((taus[b], phis[b], lo, max(0, hi - lo), metrics[b]))
        for m in range(lo, hi):
            d = soft_of(off, m)
            bits.append(ord("1") if d > 0 else ord("0"))
            soft.append(d)
            index.append((t_k(2 * m + 2, fs) + off + 65535) >> 16)
    soft = np.array(soft, dtype=F32)
    soft.view(np.uint32)[np.isnan(soft)] = 0x7FC00000                          # a NaN is stored as the quiet NaN 0x7fc00000
    return dict(bits=np.array(bits, dtype=np.uint8), soft=soft, index=np.array(index, dtype=np.int64), blocks=blocks)


def blocks_of(got) -> list:
    """an FfpBits' per-block table as the model's tuples"""
    return [(int(b["tau"]), int(b["phi"]), int(b["first_bit"]), int(b["count"]), int(b["metric"])) for b in got.blocks]


def same_as_model(got, want) -> bool:
    return (got.bits.tobytes() == want["bits"].tobytes() and got.soft.tobytes() == want["soft"].tobytes()
            and got.index.tobytes() == want["index"].tobytes() and blocks_of(got) == want["blocks"] and int(got.sync["nbits"]) == len(want["bits"])
            and int(got.sync["nblocks"]) == len(want["blocks"]))


def same_bits(a, b) -> bool:
    """two FfpBits, byte for byte: record, characters, soft bit patterns, sample indices, per-block table"""
    return (a.sync.tobytes() == b.sync.tobytes() and a.bits.tobytes() == b.bits.tobytes() and a.soft.tobytes() == b.soft.tobytes()
            and a.index.tobytes() == b.index.tobytes() and a.blocks.tobytes() == b.blocks.tobytes())


# ---------------------------------------------------------------- streams
def sent_bits(count: int, seed: int = 3) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 2, size=count).astype(np.int64)


def stream(fs: int, n: int, carrier_hz=40.0, ppm: float = 0.0, delay: float = 0.0, noise: float = 0.02, seed: int = 3, amp: float = 0.5,
           phase0: float = 0.4) -> np.ndarray:
    """n samples of a carrier at carrier_hz (a number, or an array of n instantaneous frequencies: the phase is their running sum) with
    +-1.06 rad Manchester PM of sent_bits(seed) at 8320 (1 + ppm 1e-6) bit/s, bit 0 starting `delay` samples in (zero modulation in
    front of it); bit 1 is +1.06 then -1.06 rad.  float32[n, 2]"""
    i = np.arange(n, dtype=np.float64)
    hb = np.floor((i - delay) * 16640.0 * (1.0 + ppm * 1e-6) / fs).astype(np.int64)
    bits = sent_bits(int(max(hb.max(initial=0), 0)) // 2 + 2, seed)
    b = bits[np.clip(hb // 2, 0, len(bits) - 1)]
    mod = np.where(hb >= 0, 1.06 * np.where((hb & 1) == 0, 1.0, -1.0) * np.where(b == 1, 1.0, -1.0), 0.0)
    f = np.broadcast_to(np.asarray(carrier_hz, dtype=np.float64), (n,))
    ph = 2 * np.pi * (np.cumsum(f) - f) / fs + phase0 + mod
    rng = np.random.default_rng(seed + 1000)
    z = amp * np.exp(1j * ph) + noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([z.real, z.imag], axis=1).astype(F32)


def aligned(got_bits: np.ndarray, seed: int = 3, shifts=range(-3, 4)):
    """the shift s with got[i] == sent[i + s] for every i, or None"""
    got = np.asarray(got_bits, dtype=np.int64) - ord("0")
    sent = sent_bits(len(got) + 16, seed)
    for s in shifts:
        lo = max(0, -s)
        if len(got) > lo and np.array_equal(got[lo:], sent[lo + s:len(got) + s]):
            return s
    return None


def p_samples(fs: int) -> float:
    return fs / 16640.0


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, fs, float32[n, 2] read only, cfg dict)] of the small streams: every one goes through the model (CPU) and the kernels (GPU)"""
    out = []

    def add(name, fs, y, **cfg):
        y = np.ascontiguousarray(y, dtype=F32)
        y.setflags(write=False)
        out.append((name, fs, y, dict(cfg)))

    # rates: three blocks and a bit at each
    for fs in RATES:
        L = block_len(64, fs)
        add(f"rate-{fs}", fs, stream(fs, 3 * L + int(2 * p_samples(fs)), delay=1.3 * p_samples(fs)), residual_hz=38.0, **SMALL)
    # stream lengths at 49920 (P = 3, L = 384 at B = 64)
    fs, L = 49920, 384
    for name, n in (("n0", 0), ("bit-short-of-a-block", L - 6), ("one-block", L), ("one-block-and-a-sample", L + 1)):
        add(name, fs, stream(fs, n), residual_hz=40.0, **SMALL)
    # the same, the transmitted clock half a bit off: the bit that straddles the last block's one sample does not exist, its count clamps at 0
    add("one-block-and-a-sample-half-bit-off", fs, stream(fs, L + 1, delay=3.0, noise=0.0), residual_hz=40.0, **SMALL)
    add("smoothing-window-inside", fs, stream(fs, 10 * L), residual_hz=40.0, block_bits=64, clock_steps=8, ref_bits=4)          # J = 4: 2 J + 2 blocks
    add("last-bit-ends-on-last-sample", fs, stream(fs, 2 * L), residual_hz=40.0, **SMALL)
    add("last-bit-one-sample-short", fs, stream(fs, 2 * L - 1), residual_hz=40.0, **SMALL)
    # a clock fast and slow by 2000 ppm: one step of T = 8 per block of 64 bits
    for name, ppm in (("clock-fast", 2000.0), ("clock-slow", -2000.0)):
        add(name, 50000, stream(50000, 14 * block_len(64, 50000), ppm=ppm, delay=2.0), residual_hz=40.0, block_bits=64, clock_steps=8, ref_bits=8, smooth_blocks=0)
    # a block of zeros between signal blocks, no smoothing
    y = stream(fs, 5 * L, delay=3.0, noise=0.0)
    y[2 * L:3 * L + 18] = 0.0
    add("zero-block", fs, y, residual_hz=40.0, block_bits=64, clock_steps=8, ref_bits=4, smooth_blocks=0)
    # the reference window: W = 0, and W larger than a block (clipped at both ends of the stream, straddling block seams)
    add("W0", fs, stream(fs, 3 * L), residual_hz=40.0, block_bits=64, clock_steps=8, ref_bits=0, smooth_blocks=1)
    add("W64", fs, stream(fs, 3 * L), residual_hz=40.0, block_bits=64, clock_steps=8, ref_bits=64, smooth_blocks=1)
    # Inf and NaN
    y = stream(fs, 3 * L)
    y[200, 0] = np.inf
    y[500, 1] = np.nan
    add("inf-nan", fs, y, residual_hz=40.0, **SMALL)
    # the defaults on a short stream
    add("defaults", 50000, stream(50000, 2 * block_len(208, 50000) + 77, delay=1.0), residual_hz=40.0)
    return out


NFFT_50K = 4096


@functools.lru_cache(maxsize=None)
def tone_cases():
    """[(name, fs, y, cfg)] whose residual is measured (nfft = 4096 at 50 ksps)"""
    fs, N, out = 50000, NFFT_50K, []

    def add(name, y, **cfg):
        y = np.ascontiguousarray(y, dtype=F32)
        y.setflags(write=False)
        out.append((name, fs, y, dict(cfg)))

    add("shorter-than-nfft", stream(fs, N - 1, carrier_hz=0.0))
    # two segments whose carriers differ by 30 Hz, the phase continuous, and a tail; a block's window straddles the seam
    f = np.where(np.arange(2 * N + 700) < N, -3470.0, -3500.0)
    add("seam-30hz", stream(fs, 2 * N + 700, carrier_hz=f, noise=0.01), **SMALL)
    y = stream(fs, 2 * N + 100, carrier_hz=-3470.0, noise=0.01)
    y[:N] = 0.0
    add("zero-first-segment", y, **SMALL)
    y = stream(fs, 3 * N + 100, carrier_hz=-3470.0, noise=0.01)
    y[N:2 * N] = 0.0
    add("valid-invalid-valid", y, **SMALL)
    return out
