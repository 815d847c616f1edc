"""The carrier of a channel stream as a measurement, without a GPU: pdt_host_tones against a float64 model of the same
estimator, its conventions (signed bins, the wrap at bin 0, the search set, records that are not valid), its arguments through the C
hook and through the binding, and the truth: the synthesiser's instantaneous carrier frequency in closed form and its C/N0, on the
ARGOS captures of tests/test_windows.py and tests/test_gpu_windows.py and on one POES carrier of tests/test_survey.py's capture."""
import ctypes as C
import math

import numpy as np
import pytest

from test_survey import SPECTRUM_BOUND, carriers, window64
from test_windows import ARGOS_RANGE, D, FS, IN_RATE, OFFSETS, RESIDUAL, SEEDS, platforms

NFFTS = (1024, 4096, 16384)
POES_RANGE = 4500.0
ARGOS_N = 4096                                   # the default at 32 ksps: 4096 / 32000 = 0.128 s
# Worst |freq_hz - truth| of the host hook over every burst of the two ARGOS captures (20 + 14 bursts), measured where this file was
# written: 0.0527 Hz (the two-platform capture 0.0527 Hz, the drifting platform 0.0276 Hz).  Asserted: twice that.  More than 1 Hz -- an eighth of the
# 7.8 Hz bin -- would be a defect of the estimator or of the time convention.
ARGOS_FREQ_WORST_HZ = 0.0527
ARGOS_FREQ_BOUND_HZ = 2 * ARGOS_FREQ_WORST_HZ
# The same for the segments of one POES carrier at 250 ksps, N = 16384 (15.3 Hz bins), against the constant f0: worst 0.0687 Hz
POES_FREQ_WORST_HZ = 0.0687
POES_FREQ_BOUND_HZ = 2 * POES_FREQ_WORST_HZ
CN0_MEAN_DB, CN0_EACH_DB = 1.0, 2.5              # the mean error over a capture's bursts; every burst (128 correlated bins: sigma 0.6 dB)


def as_complex(y: np.ndarray) -> np.ndarray:
    y = np.asarray(y).reshape(-1, 2)
    return y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)


def search_bins(n: int, fs: float, search_hz: float) -> np.ndarray:
    kmax = min(int(math.floor(search_hz * n / fs)), n // 2 - 1)
    return np.concatenate([np.arange(0, kmax + 1), np.arange(n - kmax, n)])


def noise_bins_of(b: int, n: int, lo: int, hi: int) -> np.ndarray:
    d = np.concatenate([-np.arange(hi, lo - 1, -1), np.arange(lo, hi + 1)])
    return (b + d) % n


def derive(bin_, below, peak, above, noise_sum, noise_bins, n, fs, offset, start):
    """The derived values of a raw record, as include/pdt.h states them, in float64."""
    w = window64(n)
    lm, l0, lp = math.log(below), math.log(peak), math.log(above)
    delta = 0.5 * (lm - lp) / (lm - 2 * l0 + lp)
    residual = ((bin_ if bin_ < n // 2 else bin_ - n) + delta) * fs / n
    power = math.exp(l0 - 0.25 * (lm - lp) * delta) / w.sum() ** 2
    cn0 = 10 * math.log10(power / (noise_sum / noise_bins / (w * w).sum()) * fs)
    return dict(time_s=(start + (n - 1) / 2) / fs, residual_hz=residual, freq_hz=offset + residual, power=power, cn0_dbhz=cn0)


def model(y: np.ndarray, n: int, fs: float, search_hz: float, first: int = 0, lo: int = 8, hi: int = 71):
    """float64: the power spectrum of the windowed segment, the peak of the search set (the lowest bin of equal ones), the noise sum."""
    P = np.abs(np.fft.fft(window64(n) * as_complex(y)[first: first + n])) ** 2
    s = np.sort(search_bins(n, fs, search_hz))
    b = int(s[np.argmax(P[s])])
    return P, b, float(P[noise_bins_of(b, n, lo, hi)].sum())


def tone(n: int, cycles_per_sample: float, amp: float = 1.0, phase: float = 0.3) -> np.ndarray:
    z = amp * np.exp(1j * (2 * np.pi * cycles_per_sample * np.arange(n) + phase))
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


@pytest.mark.parametrize("nfft", NFFTS)
def test_raw_record_matches_float64_model(pdt, nfft):
    """Full-scale random input plus a tone between two bins, two overlapping segments at an odd first sample: the bin is the model's, the
    three powers agree on tests/test_survey.py's measure within its bound, the noise sum within the bound times its bins, and the
    derived doubles are include/pdt.h's formulas on the record's own floats."""
    rng = np.random.default_rng(500 + nfft)
    fs, offset = 250000, -180000.0
    for k in (37.3, -(nfft // 8) - 0.45):
        y = (rng.uniform(-1.0, 1.0, (2 * nfft + 3, 2)) + tone(2 * nfft + 3, k / nfft)).astype(np.float32)
        got = pdt.host_tones(fs, offset, y, nfft=nfft, search_hz=0.4 * fs, first=3, stride=nfft - 5)
        assert len(got) == 2
        for i, r in enumerate(got):
            start = 3 + i * (nfft - 5)
            P, b, noise = model(y, nfft, fs, 0.4 * fs, start)
            assert r["bin"] == b == round(k) % nfft and r["valid"] == 1 and r["noise_bins"] == 128
            err = max(abs(float(r[f]) - P[(b + d) % nfft]) for f, d in (("below", -1), ("peak", 0), ("above", 1))) / P.max()
            nerr = abs(float(r["noise_sum"]) - noise) / P.max()
            print(f"nfft {nfft} k {k} segment {i}: max |p - p64| / max P64 = {err:.3e}, noise sum {nerr:.3e}")
            assert err <= SPECTRUM_BOUND and nerr <= 128 * SPECTRUM_BOUND
            want = derive(b, float(r["below"]), float(r["peak"]), float(r["above"]), float(r["noise_sum"]), 128, nfft, fs, offset, start)
            for f, v in want.items():
                assert abs(r[f] - v) <= 1e-11 * max(abs(v), 1.0), (f, r[f], v)
            assert abs(r["residual_hz"] - k * fs / nfft) < 0.1 * fs / nfft and abs(10 * math.log10(r["power"])) < 0.5


@pytest.mark.parametrize("nfft", NFFTS)
def test_conventions(pdt, nfft):
    fs = 32000
    binw = fs / nfft
    # a tone exactly on a bin's centre, both signs: |delta| < 1e-3, the signed bin
    for k in (37, -41):
        r = pdt.host_tones(fs, 1000.0, tone(nfft, k / nfft), nfft=nfft, search_hz=0.3 * fs)[0]
        assert r["valid"] == 1 and r["bin"] == k % nfft
        assert abs(r["residual_hz"] / binw - k) < 1e-3 and r["freq_hz"] == 1000.0 + r["residual_hz"]
        assert r["time_s"] == ((nfft - 1) / 2) / fs
    # bin 0: its lower neighbour is bin N - 1
    y = (tone(nfft, 0.2 / nfft) + 0.01 * np.random.default_rng(1).uniform(-1, 1, (nfft, 2))).astype(np.float32)
    r = pdt.host_tones(fs, 0.0, y, nfft=nfft, search_hz=550.0)[0]
    P, b, _ = model(y, nfft, fs, 550.0)
    assert r["bin"] == b == 0 and r["valid"] == 1
    assert abs(float(r["below"]) - P[nfft - 1]) <= SPECTRUM_BOUND * P.max() and abs(float(r["above"]) - P[1]) <= SPECTRUM_BOUND * P.max()
    assert r["below"] < r["above"] and 0.1 < r["residual_hz"] / binw < 0.3
    # the most negative bin of the search set: found there; one bin further out it is not
    kmax = 20
    y = tone(nfft, -kmax / nfft)
    r = pdt.host_tones(fs, 0.0, y, nfft=nfft, search_hz=(kmax + 0.5) * binw)[0]
    assert r["bin"] == nfft - kmax and abs(r["residual_hz"] / binw + kmax) < 1e-3
    r = pdt.host_tones(fs, 0.0, y, nfft=nfft, search_hz=(kmax - 0.5) * binw)[0]
    assert r["bin"] == nfft - kmax + 1
    # a stronger line outside the search set is not the peak
    y = (tone(nfft, 200 / nfft) + tone(nfft, 5 / nfft, amp=0.01)).astype(np.float32)
    r = pdt.host_tones(fs, 0.0, y, nfft=nfft, search_hz=(kmax + 0.5) * binw)[0]
    assert r["bin"] == 5 and r["valid"] == 1 and abs(10 * math.log10(r["power"]) + 40.0) < 0.1
    assert pdt.host_tones(fs, 0.0, y, nfft=nfft, search_hz=0.4 * fs)[0]["bin"] == 200
    # an all-zero segment: not valid, the bin's centre, a NaN C/N0
    r = pdt.host_tones(fs, 123.0, np.zeros((nfft, 2), dtype=np.float32), nfft=nfft, search_hz=550.0)[0]
    assert r["valid"] == 0 and r["bin"] == 0 and r["freq_hz"] == 123.0 and r["residual_hz"] == 0.0 and math.isnan(r["cn0_dbhz"])
    assert r["power"] == 0.0 and r["peak"] == 0.0
    # a stream shorter than N, and a first sample that leaves less than N
    assert len(pdt.host_tones(fs, 0.0, np.zeros((nfft - 1, 2), dtype=np.float32), nfft=nfft, search_hz=550.0)) == 0
    assert len(pdt.host_tones(fs, 0.0, np.zeros((nfft, 2), dtype=np.float32), nfft=nfft, search_hz=550.0, first=1)) == 0
    assert len(pdt.host_tones(fs, 0.0, np.zeros((0, 2), dtype=np.float32), nfft=nfft, search_hz=550.0)) == 0


def test_defaults_and_counts(pdt):
    """nfft: the largest allowed N with N / Fs <= 0.128 s; stride: N; count: to the end of the stream, at most cap."""
    rng = np.random.default_rng(3)
    for fs, n in ((32000, 4096), (8000, 1024), (7999, None), (150000, 16384), (250000, 16384), (32001, 4096)):
        y = rng.uniform(-1, 1, (3 * 16384 + 7, 2)).astype(np.float32)
        if n is None:
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                pdt.host_tones(fs, 0.0, y, search_hz=100.0)
            continue
        got = pdt.host_tones(fs, 0.0, y, search_hz=100.0)
        assert len(got) == len(y) // n
        assert np.array_equal(got["time_s"], (np.arange(len(got)) * n + (n - 1) / 2) / fs)
        assert got.tobytes() == pdt.host_tones(fs, 0.0, y, search_hz=100.0, nfft=n, stride=n, noise_lo=8, noise_hi=71).tobytes()
        two = pdt.host_tones(fs, 0.0, y, search_hz=100.0, count=2, first=5, stride=100)
        for i in range(2):
            one = pdt.host_tones(fs, 0.0, y[5 + 100 * i:], search_hz=100.0, count=1)[0]
            assert [one[f] for f in ("bin", "below", "peak", "above", "noise_sum")] == [two[i][f] for f in ("bin", "below", "peak", "above", "noise_sum")]
        assert len(pdt.host_tones(fs, 0.0, y, search_hz=100.0, cap=2)) == 2
    assert C.sizeof(pdt.ToneRec) == 72 == pdt.TONE_DTYPE.itemsize and C.sizeof(pdt.ToneCfg) == 48


def bad_cfgs(fs: int):
    """The PDT_ERR_ARG cases of include/pdt.h, as keyword arguments (tests/test_gpu_tones.py puts the same through a context)."""
    return [dict(nfft=2048), dict(nfft=-4096), dict(nfft=4096, search_hz=0.5 * fs), dict(nfft=4096, search_hz=-1.0),
            dict(nfft=4096, search_hz=float("nan")), dict(nfft=4096, search_hz=float("inf")), dict(nfft=4096, noise_hi=2048),
            dict(nfft=1024, noise_hi=512), dict(nfft=4096, noise_lo=72), dict(nfft=4096, noise_lo=20, noise_hi=19), dict(nfft=4096, noise_lo=-1),
            dict(nfft=4096, cap=0), dict(nfft=4096, cap=-3)]


def test_hook_and_binding_agree_on_errors(pdt):
    fs = 32000
    y = np.zeros((8192, 2), dtype=np.float32)
    L = pdt.lib()
    out, count = np.zeros(4, dtype=pdt.TONE_DTYPE), C.c_int(-7)
    for kw in bad_cfgs(fs):
        kw = dict(kw)
        cap = kw.pop("cap", 4)
        cfg = pdt.ToneCfg(**kw)
        assert L.pdt_host_tones(fs, 0.0, y.ctypes.data, len(y), C.byref(cfg), out.ctypes.data, cap, C.byref(count)) == -1, kw
        assert count.value == -7
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.host_tones(fs, 0.0, y, cap=cap, **kw)
    # ... and the good neighbours of those cases pass through both
    for kw in (dict(nfft=4096, search_hz=0.5 * fs - 1.0), dict(nfft=4096, noise_hi=2047), dict(nfft=4096, noise_lo=71), dict(nfft=1024, noise_lo=1, noise_hi=1)):
        cfg = pdt.ToneCfg(**kw)
        assert L.pdt_host_tones(fs, 0.0, y.ctypes.data, len(y), C.byref(cfg), out.ctypes.data, 4, C.byref(count)) == 0, kw
        assert count.value == len(pdt.host_tones(fs, 0.0, y, cap=4, **kw)) == min(4, 8192 // kw["nfft"])
    assert L.pdt_host_tones(0, 0.0, y.ctypes.data, len(y), None, out.ctypes.data, 4, C.byref(count)) == -1
    assert L.pdt_host_tones(fs, float("nan"), y.ctypes.data, len(y), None, out.ctypes.data, 4, C.byref(count)) == -1
    assert L.pdt_host_tones(fs, 0.0, None, len(y), None, out.ctypes.data, 4, C.byref(count)) == -1
    assert L.pdt_host_tones(fs, 0.0, y.ctypes.data, len(y), None, None, 4, C.byref(count)) == -1
    assert L.pdt_host_tones(fs, 0.0, y.ctypes.data, len(y), None, out.ctypes.data, 4, None) == -1
    with pytest.raises(TypeError):
        pdt.host_tones(fs, 0.0, y, nftt=4096)


# ---------------------------------------------------------------- the truth: the synthesiser's carrier in closed form
def signed_step(p) -> int:
    return p.carrier_step - 2 ** 32 if p.carrier_step >= 2 ** 31 else p.carrier_step


def truth_hz(p, in_rate: int, n: float) -> float:
    """The synthesiser's instantaneous carrier frequency at wideband sample n (pdt_synth_sample's phase, differentiated)."""
    return in_rate / 2 ** 32 * (signed_step(p) + p.doppler_q32 * (n - p.signal_start) / 2 ** 32)


def truth_cn0_dbhz(p, noise_params, in_rate: int) -> float:
    """A^2 / (2 sigma^2) Fs_in; per component sigma^2 = 4 (65536^2 - 1) / 12 (noise_gain / 65536)^2 + 1 / 12 (pdt_synth_noise: four 16-bit
    uniforms, scaled, rounded), added over the transmissions summed into the capture."""
    var = sum(4 * (65536 ** 2 - 1) / 12 * (q.noise_gain / 65536) ** 2 + 1 / 12 for q in noise_params)
    return 10 * math.log10(p.amplitude ** 2 / (2 * var) * in_rate)


def first_segments(pdt, x: np.ndarray, windows, n: int = ARGOS_N):
    """The first segment of every window, measured on the host: pdt_host_ddc of the slice that reaches it, then pdt_host_tones."""
    out = []
    for w in windows:
        take = min(w.nframes, (n + 16) * D)                               # (channel sample m reaches input m D + 8 D)
        y = pdt.host_ddc(IN_RATE, D, w.offset_hz, x[w.first_frame: w.first_frame + take])
        got = pdt.host_tones(FS, w.offset_hz, y, search_hz=ARGOS_RANGE, count=1)
        assert len(got) == 1 and got[0]["valid"] == 1 and got[0]["noise_bins"] == 128
        out.append(got[0])
    return out


def drifting_capture(pdt):
    """The drifting platform of tests/test_gpu_windows.py: +1200 -> -1200 Hz about 250 kHz between 2 s and 23 s of a 24 s capture."""
    secs, centre = 24.0, 250000.0
    n = int(secs * IN_RATE)
    p = pdt.synth_params(1, IN_RATE, centre, 8)
    p.amplitude //= 2
    p.noise_gain //= 2
    pdt.synth_lib().pdt_synth_set_pass(C.byref(p), 2 * IN_RATE, 23 * IN_RATE, centre + 1200.0, centre - 1200.0, 0.0)
    x = np.zeros((n, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, x.ctypes.data)
    return x, p


def check_truth(name, tones, windows, platform_of, noise_params):
    ferr, cerr = [], []
    for t, w in zip(tones, windows):
        p = platform_of(w)
        mid = w.first_frame + t["time_s"] * IN_RATE                       # channel sample m sits on input sample m D
        ferr.append(t["freq_hz"] - truth_hz(p, IN_RATE, mid))
        cerr.append(t["cn0_dbhz"] - truth_cn0_dbhz(p, noise_params, IN_RATE))
    ferr, cerr = np.array(ferr), np.array(cerr)
    print(f"{name}: {len(tones)} bursts, worst |freq_hz - truth| = {np.abs(ferr).max():.4f} Hz (mean {ferr.mean():+.4f}), "
          f"C/N0 error mean {cerr.mean():+.3f} dB, worst {np.abs(cerr).max():.3f} dB, C/N0 truth {truth_cn0_dbhz(platform_of(windows[0]), noise_params, IN_RATE):.2f} dB-Hz")
    return ferr, cerr


@pytest.fixture(scope="module")
def argos_pair_tones(pdt):
    x, params = platforms(pdt, IN_RATE, 15.0, OFFSETS, SEEDS, RESIDUAL)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, rows=False)
    windows = pdt.burst_windows(found, IN_RATE, len(x))
    return params, windows, first_segments(pdt, x, windows)


@pytest.fixture(scope="module")
def argos_drift_tones(pdt):
    x, p = drifting_capture(pdt)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, rows=False)
    windows = pdt.burst_windows(found, IN_RATE, len(x))
    return p, windows, first_segments(pdt, x, windows)


def test_argos_truth_two_platforms(pdt, argos_pair_tones):
    params, windows, tones = argos_pair_tones
    assert len(windows) == 20
    near = lambda w: params[int(np.argmin([abs(w.offset_hz - (off + RESIDUAL)) for off in OFFSETS]))]
    ferr, cerr = check_truth("two platforms", tones, windows, near, params)
    assert np.abs(ferr).max() <= ARGOS_FREQ_BOUND_HZ < 1.0
    assert abs(cerr.mean()) <= CN0_MEAN_DB and np.abs(cerr).max() <= CN0_EACH_DB


def test_argos_truth_drifting_platform(pdt, argos_drift_tones):
    p, windows, tones = argos_drift_tones
    assert len(windows) == 14
    ferr, cerr = check_truth("drifting platform", tones, windows, lambda w: p, [p])
    assert np.abs(ferr).max() <= ARGOS_FREQ_BOUND_HZ < 1.0
    assert abs(cerr.mean()) <= CN0_MEAN_DB and np.abs(cerr).max() <= CN0_EACH_DB
    f = np.array([t["freq_hz"] for t in tones])
    assert np.all(np.diff(f) < 0) and 1000.0 < f[0] - 250000.0 < 1200.0 and -1200.0 < f[-1] - 250000.0 < -1000.0      # the Doppler curve


def test_poes_carrier_at_a_stride(pdt):
    """One carrier of tests/test_survey.py's 2 s two-carrier POES capture, every segment at stride N: the residual carrier (m = 1.06
    rad: cos^2 m = -6.2 dB of the transmission's power) against the constant f0.  Its C/N0 is not asserted: the data sidebands in
    the noise bins set a ceiling."""
    in_rate, dec, offset = 1000000, 4, 200000.0
    fs = in_rate // dec
    x = carriers(pdt, 0, in_rate, 2.0, (offset, -180000.0), (11, 12), 1000.0)
    p = pdt.synth_params(0, in_rate, offset + 1000.0, 11)
    f0 = truth_hz(p, in_rate, 0)
    y = pdt.host_ddc(in_rate, dec, offset, x)
    got = pdt.host_tones(fs, offset, y, search_hz=POES_RANGE)
    assert len(got) == len(y) // 16384 == 30 and np.all(got["valid"] == 1)
    err = got["freq_hz"] - f0
    level = 10 * np.log10(got["power"] / ((p.amplitude // 2) / 32768.0) ** 2)
    print(f"POES: {len(got)} segments, worst |freq_hz - f0| = {np.abs(err).max():.4f} Hz, carrier {level.mean():+.2f} dB of the transmission, "
          f"C/N0 {got['cn0_dbhz'].min():.1f} .. {got['cn0_dbhz'].max():.1f} dB-Hz")
    assert np.abs(err).max() <= POES_FREQ_BOUND_HZ < 1.0
    assert np.all(np.abs(level - 20 * math.log10(math.cos(1.06))) < 0.5)
