"""Wideband SDR captures, host side: pdt_host_ddc -- the digital down-converter's arithmetic restated on the host, bit for bit what
the kernel runs -- against a float64 model of its definition; no GPU needed."""
import ctypes as C

import numpy as np
import pytest

DECIMS = (2, 4, 16, 64)
ALL_DECIMS = tuple(range(2, 65))                                        # everything pdt_set_channel and -x accept
FORMATS = ("pcm16", "f32", "cu8", "cs8")


def taps64(D: int) -> np.ndarray:
    """h[k] = sinc(0.8 k / D) blackman_{16 D + 1}[k + 8 D], unit sum in double, rounded to float (held as float64)."""
    n = 16 * D + 1
    k = np.arange(n) - 8 * D
    i = np.arange(n)
    w = 0.42 - 0.5 * np.cos(2 * np.pi * i / (n - 1)) + 0.08 * np.cos(4 * np.pi * i / (n - 1))
    h = np.sinc(0.8 * k / D) * w
    return (h / h.sum()).astype(np.float32).astype(np.float64)


def rot64(p: np.ndarray) -> np.ndarray:
    """e^{-j 2 pi p / 2^32} as the project's table gives it, evaluated in float64: quadrant from the top two bits, the float32 table
    of 2 pi i / 4096 for the next ten, the small-angle pair (1 - t^2 / 2, t) of the remaining twenty."""
    p = p.astype(np.uint64)
    q, r = (p >> np.uint64(30)).astype(np.int64), p & np.uint64(0x3FFFFFFF)
    hi, lo = (r >> np.uint64(20)).astype(np.int64), (r & np.uint64(0xFFFFF)).astype(np.float64)
    a = 2.0 * np.pi * np.arange(1024) / 4096.0
    ch, sh = np.cos(a).astype(np.float32).astype(np.float64)[hi], np.sin(a).astype(np.float32).astype(np.float64)[hi]
    t = lo * float(np.float32(1.46291807926715968e-09))
    cl, sl = 1.0 - 0.5 * t * t, t
    cr, sr = ch * cl - sh * sl, sh * cl + ch * sl
    c = np.choose(q, [cr, -sr, -cr, sr])
    s = np.choose(q, [sr, cr, -sr, -cr])
    return c - 1j * s


def scaled(x: np.ndarray) -> np.ndarray:
    """The capture as complex float64, scaled by format."""
    x = np.asarray(x)
    f = x.reshape(-1, 2).astype(np.float64)
    if x.dtype == np.uint8:
        f = (f - 127.5) / 128.0
    elif x.dtype == np.int8:
        f = f / 128.0
    elif x.dtype == np.int16:
        f = f / 32768.0
    return f[:, 0] + 1j * f[:, 1]


def step_of(in_rate: int, offset: float) -> int:
    return int(round(offset * 2 ** 32 / in_rate)) % 2 ** 32


def model(x: np.ndarray, in_rate: int, D: int, offset: float) -> np.ndarray:
    """float64: v = x e^{-j 2 pi p / 2^32}, y[m] = sum_k h[k] v[m D + k], v = 0 outside the capture."""
    z = scaled(x)
    N = len(z)
    p = (np.arange(N, dtype=np.uint64) * np.uint64(step_of(in_rate, offset))) % np.uint64(1 << 32)
    v = z * rot64(p)
    M = (N + D - 1) // D
    vp = np.concatenate([np.zeros(8 * D, complex), v, np.zeros(M * D + 8 * D + 1 - N, complex)])
    h = taps64(D)
    y = np.zeros(M, complex)
    for j, hk in enumerate(h):
        y += hk * vp[j: j + M * D: D]
    return y


def bound(D: int, xmax: float) -> float:
    """The fmaf chain's bound: 16 D + 1 accumulations and the roundings of the mix, each at most 2^-24 of sum |h| max|x| sqrt 2."""
    return (16 * D + 9) * 2.0 ** -24 * np.abs(taps64(D)).sum() * xmax * np.sqrt(2.0)


def capture(rng, fmt: str, n: int) -> np.ndarray:
    if fmt == "pcm16":
        return rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    if fmt == "f32":
        return rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    if fmt == "cu8":
        return rng.integers(0, 256, (n, 2)).astype(np.uint8)
    return rng.integers(-128, 128, (n, 2)).astype(np.int8)


def as_complex(y: np.ndarray) -> np.ndarray:
    return y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("D", ALL_DECIMS)
def test_host_ddc_matches_float64_model(pdt, D, fmt):
    """Every decimation the entries accept, not the powers of two alone: the host restatement is the kernel's only definition (the
    GPU tests compare the two bit for bit at every D), so it is held to the model wherever the kernel is held to it."""
    rng = np.random.default_rng(100 * D + FORMATS.index(fmt))
    in_rate = 250000 * D
    for offset in (0.37 * in_rate, -0.21 * in_rate, 1234.5):
        x = capture(rng, fmt, 40 * D + 3)
        got = as_complex(pdt.host_ddc(in_rate, D, offset, x))
        want = model(x, in_rate, D, offset)
        assert got.shape == want.shape
        err = max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag)))
        lim = bound(D, np.max(np.abs(np.concatenate([scaled(x).real, scaled(x).imag]))))
        print(f"D {D} {fmt} offset {offset:.1f}: error {err:.3e}, bound {lim:.3e}, error / bound {err / lim:.4f}")
        assert err <= lim


@pytest.mark.parametrize("D", (4, 16, 7))
def test_tone_at_the_offset_lands_at_dc_with_gain_one(pdt, D):
    """A tone at +offset and at -offset, each converted with its own sign, comes out as its amplitude at 0 Hz."""
    in_rate, amp = 250000 * D, 0.5
    n = 64 * D
    for offset in (in_rate / 8.0, -in_rate / 8.0, 0.3123 * in_rate, -0.3123 * in_rate):
        p = (np.arange(n, dtype=np.uint64) * np.uint64(step_of(in_rate, offset))) % np.uint64(1 << 32)
        tone = amp * np.exp(2j * np.pi * p.astype(np.float64) / 2 ** 32)
        x = np.stack([tone.real, tone.imag], axis=1).astype(np.float32)
        y = as_complex(pdt.host_ddc(in_rate, D, offset, x))[8: -8]
        err = max(np.max(np.abs(y.real - amp)), np.max(np.abs(y.imag)))
        lim = bound(D, amp)
        print(f"D {D} offset {offset:.1f}: |y - A| {err:.3e}, bound {lim:.3e}")
        assert err <= lim
        # with the other sign the tone lands two offsets away, in the stop band
        z = as_complex(pdt.host_ddc(in_rate, D, -offset, x))[8: -8]
        assert np.sqrt(np.mean(np.abs(z) ** 2)) <= amp * 1e-3


@pytest.mark.parametrize("D", (4, 16, 7, 33))
def test_stopband(pdt, D):
    """A tone one channel rate or more from the channel's centre comes out at least 60 dB down (the Blackman design gives about
    74 dB); the float64 model is asked first: were it to fail, the taps would be wrong."""
    in_rate, amp, offset = 250000 * D, 0.5, 0.11 * 250000 * D
    n = 96 * D
    t = np.arange(n)
    for away in (1.0, -1.0, 1.5, -1.9):                                 # (all inside the wideband: no wrap)
        f = offset + away * in_rate / D
        f = (f + in_rate / 2) % in_rate - in_rate / 2
        tone = amp * np.exp(2j * np.pi * f / in_rate * t)
        x = np.stack([tone.real, tone.imag], axis=1).astype(np.float32)
        ref = model(x, in_rate, D, offset)[8: -8]
        ref_db = 20 * np.log10(np.sqrt(np.mean(np.abs(ref) ** 2)) / amp)
        y = as_complex(pdt.host_ddc(in_rate, D, offset, x))[8: -8]
        db = 20 * np.log10(np.sqrt(np.mean(np.abs(y) ** 2)) / amp)
        print(f"D {D} tone {away:+.2f} channel rates away: model {ref_db:.1f} dB, host {db:.1f} dB")
        assert ref_db <= -60.0
        assert db <= -60.0


def test_phase_depends_on_the_global_index_only(pdt):
    """Output m depends on x[m D - 8 D .. m D + 8 D] and on m, nothing else: the outputs of a part of a capture, given the part's
    samples and its halos (the rest zero), are those of the whole capture."""
    D, in_rate, offset = 4, 1000000, 200000.0
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (3000, 2)).astype(np.float32)
    whole = pdt.host_ddc(in_rate, D, offset, x)
    for cut in (9, 100, 444):
        y = x.copy()
        y[: cut * D - 8 * D] = 0
        assert np.array_equal(pdt.host_ddc(in_rate, D, offset, y)[cut:], whole[cut:])
        y = x.copy()
        y[(cut - 1) * D + 8 * D + 1:] = 0
        assert np.array_equal(pdt.host_ddc(in_rate, D, offset, y)[:cut], whole[:cut])
    # an impulse at m D is rotated by -2 pi (step m D mod 2^32) / 2^32 and weighted with the centre tap
    imp = np.zeros((400, 2), dtype=np.float32)
    imp[50 * D, 0] = 1.0
    z = as_complex(pdt.host_ddc(in_rate, D, offset, imp))[50]
    want = taps64(D)[8 * D] * np.exp(-2j * np.pi * ((50 * D * step_of(in_rate, offset)) % 2 ** 32) / 2 ** 32)
    assert abs(z - want) <= 1e-6


@pytest.mark.parametrize("D", ALL_DECIMS)
def test_output_count(pdt, D):
    rng = np.random.default_rng(D)
    for n in (0, 1, D - 1, D, D + 1, 8 * D - 1, 8 * D, 8 * D + 1, 23 * D - 1, 23 * D, 23 * D + 1):
        x = capture(rng, "pcm16", n)
        y = pdt.host_ddc(250000 * D, D, 1000.0, x)
        assert y.shape == ((n + D - 1) // D, 2)
        if n:
            d = as_complex(y) - model(x, 250000 * D, D, 1000.0)
            assert max(np.max(np.abs(d.real)), np.max(np.abs(d.imag))) <= bound(D, 1.0)


def test_scalings_are_exact(pdt):
    """A capture of one sample at offset 0 leaves y[0] = fl(h[0] x[0]): the 8-bit and 16-bit scalings, exactly."""
    D, in_rate = 4, 1000000
    hc = pdt.host_ddc(in_rate, D, 0.0, np.array([[1.0, 0.0]], dtype=np.float32))[0, 0]
    assert hc == np.float32(taps64(D)[8 * D])
    for u in range(256):
        y = pdt.host_ddc(in_rate, D, 0.0, np.array([[u, 255 - u]], dtype=np.uint8))[0]
        assert y[0] == hc * np.float32((u - 127.5) / 128.0) and y[1] == hc * np.float32((255 - u - 127.5) / 128.0)
        s = u - 128
        y = pdt.host_ddc(in_rate, D, 0.0, np.array([[s, -1 - s]], dtype=np.int8))[0]
        assert y[0] == hc * np.float32(s / 128.0) and y[1] == hc * np.float32((-1 - s) / 128.0)
    for s in (-32768, -12345, -1, 0, 1, 777, 32767):
        y = pdt.host_ddc(in_rate, D, 0.0, np.array([[s, -1 - s]], dtype=np.int16))[0]
        assert y[0] == hc * np.float32(s / 32768.0) and y[1] == hc * np.float32((-1 - s) / 32768.0)


def test_bad_arguments(pdt):
    L = pdt.lib()
    x = np.zeros(64, dtype=np.int16)
    out = np.zeros(64, dtype=np.float32)
    assert L.pdt_host_ddc(1000000, 4, 200000.0, x.ctypes.data, 32, pdt.FMT_WB_PCM16, out.ctypes.data) == 0
    for rate, decim, off, fmt in ((1000000, 1, 0.0, 16), (1000000, 65, 0.0, 16), (1000000, 0, 0.0, 16), (1000000, -4, 0.0, 16),
                                  (1000000, 4, 500000.0, 16), (1000000, 4, -500000.0, 16), (1000000, 4, float("nan"), 16),
                                  (1000000, 4, float("inf"), 17), (0, 4, 0.0, 16), (1000000, 4, 0.0, 0), (1000000, 4, 0.0, 1),
                                  (1000000, 4, 0.0, 2), (1000000, 4, 0.0, 3), (1000000, 4, 0.0, 15), (1000000, 4, 0.0, 20)):
        assert L.pdt_host_ddc(rate, decim, off, x.ctypes.data, 8, fmt, out.ctypes.data) == -1, (rate, decim, off, fmt)
    assert L.pdt_host_ddc(1000000, 4, 499999.0, x.ctypes.data, 8, 16, out.ctypes.data) == 0
    assert L.pdt_host_ddc(1000000, 4, 0.0, None, 8, 16, out.ctypes.data) == -1
    assert L.pdt_host_ddc(1000000, 4, 0.0, x.ctypes.data, 8, 16, None) == -1
    assert L.pdt_host_ddc(1000000, 4, 0.0, None, 0, 16, None) == 0
    # the context entries check their arguments before they need a GPU
    n = C.c_uint64(0)
    assert L.pdt_set_channel(None, 4, 0.0) == -1
    assert L.pdt_demod_channel(None, x.ctypes.data, 8, 16) == -1
    assert L.pdt_demod_device_channel(None, x.ctypes.data, 8, 16) == -1
    assert L.pdt_demod_channels_device(None, 2, x.ctypes.data, 8, 16) == -1
    assert L.pdt_demod_channels(None, 2, x.ctypes.data, 8, 16) == -1
    assert L.pdt_stream_push_channel(None, x.ctypes.data, 8, 16, C.byref(n)) == -1
