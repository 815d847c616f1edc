"""The carrier survey of wideband captures, host side: pdt_host_survey -- the survey's arithmetic restated on the host, bit for bit what
the kernels run -- against a float64 model of its definition, and the carriers it finds in captures of the synthetic
generator against the carriers sent; no GPU needed."""
import ctypes as C

import numpy as np
import pytest

FORMATS = ("pcm16", "f32", "cu8", "cs8")
NFFTS = (1024, 4096, 16384)
RUN = 64                                                                # SURVEY_RUN of csrc/pdt_survey.h
POES_RANGE, ARGOS_RANGE = 4500.0, 550.0                                 # the modes' PLL frequency ranges: the default merge_hz

# tests/test_gpu_channel_input.py::SETUPS and its construction of a capture, restated (that module needs a GPU to import its kin)
SETUPS = [(1000000, 4, (200000.0, -180000.0)), (2400000, 16, (600000.0, -400000.0)), (2048000, 8, (299500.0, -421700.0))]


def carriers(pdt, kind: int, in_rate: int, secs: float, offsets, seeds, residual: float, divide=None):
    """Transmissions summed into one int16 capture at in_rate, the carrier of channel i at offsets[i] + residual, its amplitude
    divided by divide[i] (2 when not given: half amplitude each, as the GPU tests build theirs), the noise by 2."""
    n = int(round(secs * in_rate))
    total = np.zeros((n, 2), dtype=np.int32)
    for i, (off, seed) in enumerate(zip(offsets, seeds)):
        p = pdt.synth_params(kind, in_rate, off + residual, seed)
        p.amplitude //= divide[i] if divide else 2
        p.noise_gain //= 2
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
        total += iq
    return np.clip(total, -32768, 32767).astype(np.int16)


def to_cu8(x16: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(x16 / 256.0) + 128, 0, 255).astype(np.uint8)


def capture(rng, fmt: str, n: int) -> np.ndarray:
    if fmt == "pcm16":
        return rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    if fmt == "f32":
        return rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    if fmt == "cu8":
        return rng.integers(0, 256, (n, 2)).astype(np.uint8)
    return rng.integers(-128, 128, (n, 2)).astype(np.int8)


def scaled(x: np.ndarray) -> np.ndarray:
    f = x.reshape(-1, 2).astype(np.float64)
    if x.dtype == np.uint8:
        f = (f - 127.5) / 128.0
    elif x.dtype == np.int8:
        f = f / 128.0
    elif x.dtype == np.int16:
        f = f / 32768.0
    return f[:, 0] + 1j * f[:, 1]


def window64(n: int) -> np.ndarray:
    """The Blackman window of n points, in double, rounded to float (held as float64)."""
    i = np.arange(n)
    return (0.42 - 0.5 * np.cos(2 * np.pi * i / (n - 1)) + 0.08 * np.cos(4 * np.pi * i / (n - 1))).astype(np.float32).astype(np.float64)


def model(x: np.ndarray, nfft: int) -> np.ndarray:
    """float64: the mean over the whole segments of |fft(w x)|^2."""
    z = scaled(x)
    nseg = len(z) // nfft
    seg = z[: nseg * nfft].reshape(nseg, nfft) * window64(nfft)
    return np.mean(np.abs(np.fft.fft(seg, axis=1)) ** 2, axis=0)


# max |P - P64| / max P64 of the host hook on the inputs of the test below, the worst case of each NFFT over the formats and lengths
# (measured; the bound is four times the worst of them: float32 FFT error grows with log NFFT and with the input's crest):
#   NFFT  1024: 3.23e-07 (pcm16, 66 segments)    NFFT  4096: 3.88e-07 (cu8, 66 segments)    NFFT 16384: 3.44e-07 (cu8, 66 segments)
SPECTRUM_BOUND = 4 * 3.88e-07


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nfft", NFFTS)
def test_spectrum_matches_float64_model(pdt, nfft, fmt):
    rng = np.random.default_rng(10 * nfft + FORMATS.index(fmt))
    for nseg, extra in ((1, 0), (3, 17), (RUN + 2, nfft - 1)):
        if nseg > 3 and nfft == 16384 and fmt != "cu8":
            continue                                                    # (one long case of the largest transform is enough)
        x = capture(rng, fmt, nseg * nfft + extra)
        got, _ = pdt.host_survey(1000000, POES_RANGE, 250000, x, nfft=nfft)
        want = model(x, nfft)
        err = np.max(np.abs(got.astype(np.float64) - want)) / np.max(want)
        print(f"nfft {nfft} {fmt} {nseg} segment(s): max |P - P64| / max P64 = {err:.3e}")
        assert err <= SPECTRUM_BOUND


@pytest.mark.parametrize("nfft", NFFTS)
def test_tone_on_a_bin_peaks_there_with_the_windows_leakage(pdt, nfft):
    """A complex exponential exactly on bin k, both signs: the peak is bin k and the spectrum around it is the float64 model's, that
    is the Blackman window's.  On a bin the main lobe is five bins wide (0, -4.5, -20.4 dB) and the side lobes are sampled near
    their nulls, 96 dB down; half-way between two bins they show at their full height, the window's 58 dB.  Every figure is asserted
    against the model.  Bounds: the transform's amplitude error is some 2 x 2^-24 log2(N) of the peak's, 115 dB under it at N = 16384;
    that moves a bin 20 dB down by less than 0.001 dB and one 58 dB down by 0.02 dB: 0.05 dB for the main lobe and for the full side
    lobe.  A sampled null, 96 to 120 dB down, is of that error's own size: it may stand at the model's amplitude plus that error."""
    n = np.arange(nfft)
    out = [0, 1, 2, 3, 4, 12, 13, 14, 15, 16]                           # of the 17 bins around the peak: those outside the main lobe
    for k in (100, -100, nfft // 2 - 7, -(nfft // 2) + 7):
        tone = 0.5 * np.exp(2j * np.pi * k * n / nfft)
        x = np.stack([tone.real, tone.imag], axis=1).astype(np.float32)
        got, found = pdt.host_survey(1000000, POES_RANGE, 250000, x, nfft=nfft)
        want = model(x, nfft)
        b = k % nfft
        assert int(np.argmax(got)) == b == int(np.argmax(want))
        rel = 10 * np.log10(np.roll(got.astype(np.float64), -b + 8)[:17] / got[b])
        rel64 = 10 * np.log10(np.roll(want, -b + 8)[:17] / want[b])
        print(f"nfft {nfft} k {k}: main lobe {rel[6:11].round(2)}, side lobes at the bins {rel[out].max():.2f} dB (model {rel64[out].max():.2f} dB)")
        assert np.max(np.abs(rel[6:11] - rel64[6:11])) <= 0.05
        assert np.all(rel[out] <= 20 * np.log10(10 ** (rel64[out] / 20) + 10 ** (-115.0 / 20)))
        assert abs(found[0].offset_hz - k * 1000000 / nfft) <= 1e-3 * 1000000 / nfft
        # half a bin up: the side lobes at their full height
        tone = 0.5 * np.exp(2j * np.pi * (k + 0.5) * n / nfft)
        x = np.stack([tone.real, tone.imag], axis=1).astype(np.float32)
        got, _ = pdt.host_survey(1000000, POES_RANGE, 250000, x, nfft=nfft)
        want = model(x, nfft)
        rel = 10 * np.log10(np.roll(got.astype(np.float64), -b + 8)[:18] / got.max())
        rel64 = 10 * np.log10(np.roll(want, -b + 8)[:18] / want.max())
        far = [0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17]
        print(f"nfft {nfft} k {k} + 1/2: highest side lobe {rel[far].max():.2f} dB (model {rel64[far].max():.2f} dB)")
        assert abs(rel[far].max() - rel64[far].max()) <= 0.05


def test_a_stretch_is_the_copied_out_stretch(pdt):
    """first_frame / nframes of a longer capture = the survey of the copy, spectrum bytes and carriers alike; the trailing partial
    segment changes nothing."""
    in_rate, nfft = 1000000, 4096
    x = carriers(pdt, 0, in_rate, 1.0, (200000.0, -180000.0), (11, 12), 1000.0)
    for first, n in ((0, 70 * nfft), (12345, 66 * nfft + 100), (len(x) - 3 * nfft, 3 * nfft)):
        a = pdt.host_survey(in_rate, POES_RANGE, 250000, x, nfft=nfft, first_frame=first, nframes=n)
        b = pdt.host_survey(in_rate, POES_RANGE, 250000, x[first: first + n].copy(), nfft=nfft)
        c = pdt.host_survey(in_rate, POES_RANGE, 250000, x[first: first + n // nfft * nfft].copy(), nfft=nfft)
        assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1] == b[1] == c[1]
        assert len(a[1]) == 2
    # nframes = 0: to the end
    a = pdt.host_survey(in_rate, POES_RANGE, 250000, x, nfft=nfft, first_frame=500000)
    b = pdt.host_survey(in_rate, POES_RANGE, 250000, x[500000:].copy(), nfft=nfft)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("rendering", ["pcm16", "cu8"])
@pytest.mark.parametrize("nfft", (4096, 16384))
@pytest.mark.parametrize("in_rate,D,offsets", SETUPS)
def test_poes_carriers_found_are_the_carriers_sent(pdt, in_rate, D, offsets, nfft, rendering):
    """Two POES transmissions, 2 s: exactly two carriers, each within one bin width of offset + 1000 Hz (the peak bin with a centroid
    around it is a sub-bin estimate)."""
    x = carriers(pdt, 0, in_rate, 2.0, offsets, (11, 12), 1000.0)
    if rendering == "cu8":
        x = to_cu8(x)
    _, found = pdt.host_survey(in_rate, POES_RANGE, in_rate // D, x, nfft=nfft)
    print(in_rate, D, nfft, rendering, [(round(c.offset_hz, 1), round(c.peak_db, 1)) for c in found])
    assert len(found) == 2
    assert found[0].peak_db >= found[1].peak_db
    for off in offsets:
        assert min(abs(c.offset_hz - (off + 1000.0)) for c in found) <= in_rate / nfft


@pytest.mark.parametrize("threshold", (10.0, 15.0, 20.0))
def test_unequal_carriers_are_both_found(pdt, threshold):
    in_rate, offsets = 1000000, (200000.0, -180000.0)
    x = carriers(pdt, 0, in_rate, 2.0, offsets, (11, 12), 1000.0, divide=(2, 16))
    _, found = pdt.host_survey(in_rate, POES_RANGE, 250000, x, threshold_db=threshold)
    print(threshold, [(round(c.offset_hz, 1), round(c.peak_db, 1)) for c in found])
    assert len(found) == 2
    assert abs(found[0].offset_hz - 201000.0) <= in_rate / 16384 and abs(found[1].offset_hz + 179000.0) <= in_rate / 16384
    assert found[0].peak_db > found[1].peak_db >= threshold


def test_noise_only_has_no_carrier(pdt):
    in_rate, n = 1000000, 2000000
    p = pdt.synth_params(0, in_rate, 1000.0, 5)
    p.amplitude = 0
    x = np.zeros((n, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, x.ctypes.data)
    assert np.std(x.astype(np.float64)) > 10.0                           # (there is noise)
    spec, found = pdt.host_survey(in_rate, POES_RANGE, 250000, x)
    print(f"strongest bin {10 * np.log10(spec.max() / np.median(spec)):.2f} dB over the median")
    assert len(found) == 0


def test_argos_carrier(pdt):
    """One ARGOS transmission at 1.024 Msps, 20 s: the strongest carrier is within one bin of 100 120 Hz.  With the default guard (half
    the channel rate, 16 kHz) the bursts' data energy just outside the guard may come up as a second peak at the threshold; a guard of
    the full channel rate leaves the carrier alone."""
    in_rate, D = 1024000, 32
    x = carriers(pdt, 1, in_rate, 20.0, (100000.0,), (8,), 120.0)
    _, found = pdt.host_survey(in_rate, ARGOS_RANGE, in_rate // D, x)
    print([(round(c.offset_hz, 1), round(c.peak_db, 1)) for c in found])
    assert len(found) >= 1 and abs(found[0].offset_hz - 100120.0) <= in_rate / 16384
    _, found = pdt.host_survey(in_rate, ARGOS_RANGE, in_rate // D, x, guard_hz=float(in_rate // D))
    print([(round(c.offset_hz, 1), round(c.peak_db, 1)) for c in found])
    assert len(found) == 1 and abs(found[0].offset_hz - 100120.0) <= in_rate / 16384


def test_max_carriers_and_capacity(pdt):
    in_rate = 1000000
    x = carriers(pdt, 0, in_rate, 1.0, (200000.0, -180000.0), (11, 12), 1000.0)
    _, both = pdt.host_survey(in_rate, POES_RANGE, 250000, x, nfft=4096)
    _, one = pdt.host_survey(in_rate, POES_RANGE, 250000, x, nfft=4096, max_carriers=1)
    assert len(both) == 2 and one == both[:1]
    L = pdt.lib()
    rec, count = (pdt.CarrierRec * 1)(), C.c_int(-1)
    cfg = pdt.SurveyCfg(nfft=4096)
    assert L.pdt_host_survey(in_rate, POES_RANGE, 250000, pdt.FMT_WB_PCM16, x.ctypes.data, len(x), C.byref(cfg), None, rec, 1, C.byref(count)) == 0
    assert count.value == 1 and rec[0].offset_hz == both[0].offset_hz


def test_bad_arguments(pdt):
    L = pdt.lib()
    x = np.zeros((2 * 16384, 2), dtype=np.int16)
    spec = np.zeros(16384, dtype=np.float32)
    rec, count = (pdt.CarrierRec * 16)(), C.c_int(0)

    def call(fmt=16, n=len(x), cap=16, data=x.ctypes.data, found=rec, cnt=C.byref(count), rate=1000000, chan=250000, rng=4500.0, **cfg):
        c = pdt.SurveyCfg(**cfg)
        return L.pdt_host_survey(rate, rng, chan, fmt, data, n, C.byref(c), spec.ctypes.data, found, cap, cnt)

    assert call() == 0 and count.value == 0
    assert L.pdt_host_survey(1000000, 4500.0, 250000, 16, x.ctypes.data, len(x), None, None, rec, 16, C.byref(count)) == 0
    for nfft in (1024, 4096, 16384):
        assert call(nfft=nfft) == 0
    for fmt in (0, 1, 2, 3, 15, 20):
        assert call(fmt=fmt) == -1                                      # not a wideband format
    for nfft in (1, 512, 1000, 2048, 8192, 32768, -1024):
        assert call(nfft=nfft) == -1
    assert call(n=16383) == -1                                          # shorter than one segment
    assert call(n=16384) == 0
    assert call(nfft=1024, n=1023) == -1
    assert call(first_frame=len(x) - 16383) == -1
    assert call(first_frame=len(x) - 16384) == 0
    assert call(first_frame=len(x) + 1) == -1                           # a stretch outside the capture
    assert call(first_frame=16384, nframes=16385) == -1
    assert call(nframes=16383) == -1
    assert call(cap=0) == -1 and call(cap=-1) == -1
    assert call(max_carriers=-1) == -1
    assert call(guard_hz=-1.0) == -1 and call(merge_hz=float("nan")) == -1 and call(threshold_db=float("inf")) == -1
    assert call(rate=0) == -1 and call(chan=0) == -1 and call(rng=0.0) == -1
    assert call(data=None) == -1 and call(found=None) == -1 and call(cnt=None) == -1
    # the context entries check their arguments before they need a GPU
    assert L.pdt_survey(None, x.ctypes.data, len(x), 16, None, rec, 16, C.byref(count)) == -1
    assert L.pdt_survey_device(None, x.ctypes.data, len(x), 16, None, rec, 16, C.byref(count)) == -1
    assert L.pdt_survey_spectrum(None, spec.ctypes.data, 16384) == -1
