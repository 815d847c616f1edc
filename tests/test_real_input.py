"""Single-channel (real) captures, host side: pdt_host_analytic -- the Hilbert front end's arithmetic restated on the host, bit
for bit what the kernel runs -- against a float64 model of its definition; no GPU needed."""
import ctypes as C

import numpy as np
import pytest

D = 31
K = np.arange(1, D + 1, 2)


def model(x: np.ndarray, fs: int, center: float) -> np.ndarray:
    """float64: Q[n] = sum_k h[k] (x[n-k] - x[n+k]) with the float taps, a = x + jQ, z = a e^{-j 2 pi p / 2^32}."""
    n = np.arange(63)
    w = 0.42 - 0.5 * np.cos(2 * np.pi * n / 62) + 0.08 * np.cos(4 * np.pi * n / 62)
    h = (2.0 / (np.pi * K) * w[K + D]).astype(np.float32).astype(np.float64)
    xp = np.concatenate([np.zeros(D), x.astype(np.float64), np.zeros(D)])
    N = len(x)
    q = np.zeros(N)
    for hk, k in zip(h, K):
        q += hk * (xp[D - k: D - k + N] - xp[D + k: D + k + N])
    step = (1 << 30) if center == 0 else int(round(center * 2 ** 32 / fs))
    p = (np.arange(N, dtype=np.uint64) * np.uint64(step)) % np.uint64(1 << 32)
    phi = 2 * np.pi * p.astype(np.float64) / 2 ** 32
    return (x + 1j * q) * np.exp(-1j * phi)


def as_complex(z: np.ndarray) -> np.ndarray:
    return z[:, 0].astype(np.float64) + 1j * z[:, 1].astype(np.float64)


@pytest.mark.parametrize("fs,center", [(96000, 0.0), (96000, 24000.0), (96000, 23456.7), (96000, 1000.0), (96000, 47000.0),
                                       (250000, 0.0), (250000, 31234.5), (32000, 7777.0)])
def test_host_analytic_matches_float64_model(pdt, fs, center):
    rng = np.random.default_rng(int(center) + fs)
    n = 5000
    x16 = rng.integers(-32768, 32768, n).astype(np.int16)           # full scale
    got = as_complex(pdt.host_analytic(fs, center, x16))
    assert np.max(np.abs(got - model(x16 / 32768.0, fs, center))) <= 2e-6
    xf = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    got = as_complex(pdt.host_analytic(fs, center, xf))
    assert np.max(np.abs(got - model(xf.astype(np.float64), fs, center))) <= 2e-6


def test_quarter_rate_centre_is_a_swap_and_negation(pdt):
    """At Fs / 4 the rotation is exactly (1, 0), (0, 1), (-1, 0), (0, -1): z is (x, Q), (Q, -x), (-x, -Q), (-Q, x) exactly."""
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, 4001).astype(np.int16)
    z = pdt.host_analytic(96000, 0.0, x)
    assert np.array_equal(z, pdt.host_analytic(96000, 24000.0, x))       # 0 means Fs / 4
    xf = (x / 32768.0).astype(np.float32)
    n = np.arange(len(x)) % 4
    qq = np.empty(len(x), dtype=np.float32)
    qq[n == 0], qq[n == 1], qq[n == 2], qq[n == 3] = z[n == 0, 1], z[n == 1, 0], -z[n == 2, 1], -z[n == 3, 0]
    assert np.array_equal(z[n == 0, 0], xf[n == 0]) and np.array_equal(z[n == 1, 1], -xf[n == 1])
    assert np.array_equal(z[n == 2, 0], -xf[n == 2]) and np.array_equal(z[n == 3, 1], xf[n == 3])
    # the other component is Q itself, so |z| = |a| up to rounding
    q_model = (model(x / 32768.0, 96000, 0) * np.exp(0.5j * np.pi * np.arange(len(x)))).imag
    assert np.max(np.abs(qq - q_model)) <= 2e-6
    assert np.max(np.abs(np.abs(as_complex(z)) - np.hypot(xf, qq))) <= 1e-6


def test_phase_depends_on_the_global_index_only(pdt):
    """Output n depends on x[n - 31 .. n + 31] and on n, nothing else: the outputs of a part of a capture, given the part's samples
    and its halo (the rest zero), are those of the whole capture -- what the kernel relies on when it converts a capture in
    segments or stream pushes from their global index."""
    fs, center = 96000, 23456.7
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, 3000).astype(np.float32)
    whole = pdt.host_analytic(fs, center, x)
    # the same samples with the first `cut` replaced by zeros except the last 31 of them (the left halo): outputs >= cut unchanged
    for cut in (31, 100, 1777):
        y = x.copy()
        y[: cut - D] = 0
        part = pdt.host_analytic(fs, center, y)
        assert np.array_equal(part[cut:], whole[cut:])
        # and the outputs < cut with the right halo only
        y = x.copy()
        y[cut + D:] = 0
        part = pdt.host_analytic(fs, center, y)
        assert np.array_equal(part[:cut], whole[:cut])
    # an impulse at n is rotated by -2 pi (step n mod 2^32) / 2^32, wherever the capture starts
    step = int(round(center * 2 ** 32 / fs))
    imp = np.zeros(200, dtype=np.float32)
    imp[150] = 1.0
    z = as_complex(pdt.host_analytic(fs, center, imp))[150]
    assert abs(z - np.exp(-2j * np.pi * ((150 * step) % 2 ** 32) / 2 ** 32)) <= 1e-6


@pytest.mark.parametrize("fs,center", [(96000, 0.0), (96000, 23456.7), (250000, 62500.0), (32000, 8000.0)])
def test_image_rejection_tone_sweep(pdt, fs, center):
    """A real tone at centre + delta leaves a line at +delta and an image at -delta; over [0.05, 0.45] Fs the image is >= 70 dB down."""
    n = 8192
    t = np.arange(n)
    win = np.blackman(n)
    for f in np.linspace(0.05, 0.45, 33) * fs:
        x = (0.5 * np.cos(2 * np.pi * f / fs * t)).astype(np.float32)
        z = as_complex(pdt.host_analytic(fs, center, x))[64:-64]
        m = np.arange(len(z))
        delta = f - (fs / 4 if center == 0 else center)
        if abs(delta) < 0.01 * fs:
            continue                                 # (the line and its image are one)
        wanted = abs(np.sum(win[64:-64] * z * np.exp(-2j * np.pi * delta / fs * m)))
        image = abs(np.sum(win[64:-64] * z * np.exp(2j * np.pi * delta / fs * m)))
        assert 20 * np.log10(image / wanted) <= -70, f"f = {f:.0f} Hz: image {20 * np.log10(image / wanted):.1f} dB"


def test_bad_arguments(pdt):
    L = pdt.lib()
    x = np.zeros(16, dtype=np.int16)
    out = np.zeros(32, dtype=np.float32)
    ok = L.pdt_host_analytic(96000, 0.0, x.ctypes.data, 16, 2, out.ctypes.data)
    assert ok == 0
    for fs, c, fmt in ((96000, 48000.0, 2), (96000, -1.0, 2), (96000, float("nan"), 2), (96000, float("inf"), 3),
                       (0, 0.0, 2), (96000, 0.0, 0), (96000, 0.0, 1), (96000, 0.0, 4)):
        assert L.pdt_host_analytic(fs, c, x.ctypes.data, 16, fmt, out.ctypes.data) == -1, (fs, c, fmt)
    assert L.pdt_host_analytic(96000, 0.0, None, 16, 2, out.ctypes.data) == -1
    assert L.pdt_host_analytic(96000, 0.0, x.ctypes.data, 16, 2, None) == -1
    assert L.pdt_host_analytic(96000, 0.0, None, 0, 2, None) == 0
    # the context entries check their arguments before they need a GPU
    assert L.pdt_set_real_input(None, 0.0) == -1
    assert L.pdt_demod_real(None, x.ctypes.data, 16, 2) == -1
    assert L.pdt_demod_device_real(None, x.ctypes.data, 16, 2) == -1
    n = C.c_uint64(0)
    assert L.pdt_stream_push_real(None, x.ctypes.data, 16, 2, C.byref(n)) == -1
