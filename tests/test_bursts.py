"""Short transmissions in a wideband capture, host side: pdt_host_bursts -- the waterfall, the rows' peaks and their linking into
bursts restated on the host, bit for bit what the kernels and the context run -- against a float64 model of the rows
and against gated tones whose times and offsets are known; no GPU needed."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_survey import FORMATS, NFFTS, SPECTRUM_BOUND, capture, scaled, window64

ARGOS_RANGE = 550.0
IN_RATE, FS = 1000000, 31250                                            # a wideband capture and the channel rate of its contexts (decim 32)


def model_rows(x: np.ndarray, nfft: int, per: int) -> np.ndarray:
    """float64: row t = the sum over its `per` segments of |fft(w x)|^2."""
    z = scaled(x)
    nrows = len(z) // (nfft * per)
    seg = z[: nrows * per * nfft].reshape(nrows, per, nfft) * window64(nfft)
    return np.sum(np.abs(np.fft.fft(seg, axis=2)) ** 2, axis=1)


def noise(rng, n: int, sigma: float) -> np.ndarray:
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def tone_amplitude(nfft: int, sigma: float, strength: float) -> float:
    """The amplitude of a tone on a bin's centre whose bin stands `strength` times over the mean noise power of a bin: the tone's bin
    holds A^2 (sum w)^2, a noise bin 2 sigma^2 sum w^2 on average."""
    w = window64(nfft)
    return float(np.sqrt(strength * 2 * sigma ** 2 * np.sum(w ** 2)) / np.sum(w))


def pairs(z: np.ndarray) -> np.ndarray:
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


def gated(rng, nfft: int, per: int, nrows: int, extra: int, sigma: float, platforms):
    """Noise plus, per platform (bin, amplitude, [(first row, rows), ...]), a tone on that bin's centre during its bursts (rows may be
    fractions)."""
    n = nrows * per * nfft + extra
    t = np.arange(n)
    z = noise(rng, n, sigma)
    for b, amp, bursts in platforms:
        on = np.zeros(n, dtype=bool)
        for first, rows in bursts:
            on[int(first * per * nfft): int((first + rows) * per * nfft)] = True
        z += on * amp * np.exp(2j * np.pi * b * t / nfft)
    return pairs(z)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nfft", NFFTS)
def test_rows_match_float64_model(pdt, nfft, fmt):
    """Full-scale random input, R = 1, 8 and 64, a partial segment and a partial row behind the last row.  The arithmetic of a
    segment is the survey's and a row is a plain float sum of at most 64 of them, so the bound is the one tests/test_survey.py
    asserts for the averaged spectrum against its float64 model, on the same measure: max |W - W64| / max W64."""
    rng = np.random.default_rng(7 * nfft + FORMATS.index(fmt))
    for per, nrows in ((1, 3), (8, 2), (64, 1)):
        if per == 64 and nfft == 16384 and fmt != "cu8":
            continue                                                    # (one long case of the largest transform is enough)
        x = capture(rng, fmt, nrows * per * nfft + (per - 1) * nfft + 17 if per > 1 else nrows * nfft + 17)
        got, _, _, _ = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per)
        want = model_rows(x, nfft, per)
        assert got.shape == want.shape == (nrows, nfft)
        err = np.max(np.abs(got.astype(np.float64) - want)) / np.max(want)
        print(f"nfft {nfft} {fmt} R {per}: max |W - W64| / max W64 = {err:.3e}")
        assert err <= SPECTRUM_BOUND


def test_spectra_digests(pdt):
    """The bits of pdt_host_survey's spectrum and carriers and of pdt_host_bursts' rows, peaks, counts and bursts are those of the
    commit that tests/golden/spectra_digests.json names, on the seeded inputs of tests/golden/make_spectra_digests.py: four formats,
    three NFFT, a survey of 197 segments and 77 samples whole and as a stretch, burst searches at R = 1, 3, 8 and 64 that end with a
    partial row and a partial segment.  An input whose own digest differs is reported as such: then numpy moved, not the library."""
    spec = importlib.util.spec_from_file_location("make_spectra_digests", os.path.join(GOLDEN, "make_spectra_digests.py"))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    with open(os.path.join(GOLDEN, "spectra_digests.json")) as f:
        want = json.load(f)["digests"]
    got = make.digests(pdt)
    assert sorted(got) == sorted(want) and len(want) == 12 * (2 + 4)
    assert [k for k in want if got[k]["input"] != want[k]["input"]] == [], "the test's own inputs differ"
    assert [k for k in want if got[k] != want[k]] == []
    assert all(want[k]["ncarriers"] >= 1 for k in want if k.startswith("survey"))
    assert all(want[k]["npeaks"] >= 1 and want[k]["nbursts"] >= 1 for k in want if k.startswith("bursts"))


def test_gated_tones_in_noise(pdt):
    """Two platforms, four bursts: one starts in the middle of a row, one lasts to the end of the stretch.  Every burst is found,
    its start within one row, its length within two rows, its offset within one bin, and the platforms are exactly the two."""
    nfft, per, nrows, sigma = 4096, 8, 40, 0.05
    binw, row_s = IN_RATE / nfft, per * nfft / IN_RATE
    amp = tone_amplitude(nfft, sigma, 1000.0)                          # 30 dB over the floor while on
    plat = [(410, amp, [(5.5, 6.5), (25, 6)]), (nfft - 820, amp, [(15, 7), (34, 6)])]
    x = gated(np.random.default_rng(21), nfft, per, nrows, 1234, sigma, plat)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per)
    want = sorted((first * row_s, rows * row_s, (b if b < nfft // 2 else b - nfft) * binw) for b, _, bursts in plat for first, rows in bursts)
    assert len(found) == len(want) == 4
    for f, (start, length, off) in zip(found, want):
        print(f, start, length, off)
        assert abs(f.start_s - start) <= row_s and abs(f.duration_s - length) <= 2 * row_s and abs(f.offset_hz - off) <= binw
        assert f.start_s == f.first_row * per * nfft / IN_RATE and f.duration_s == f.rows * per * nfft / IN_RATE
    assert found[-1].first_row + found[-1].rows == nrows               # the one that touches the end
    car = pdt.burst_carriers(found, ARGOS_RANGE)
    assert len(car) == 2
    assert sorted(round(c.offset_hz / binw) for c in car) == [-820, 410]
    assert car[0].peak_db >= car[1].peak_db


def test_rare_bursts_the_survey_cannot_see(pdt):
    """What the burst search exists for.  One platform sends two bursts of two rows each in 400 rows: duty d = 0.01.  While it is on
    its bin holds S = 400 times the mean noise power of a bin: 1 + S = 26.0 dB over the floor, 11 dB over the 15 dB threshold;
    averaged over the stretch the bin holds 1 + d S = 5 times the floor, 7.0 dB, 8 dB under the threshold.  Both margins (6 dB over,
    4 dB under) are checked on what the hook computes before anything else; then the survey finds no carrier and the burst search
    finds both bursts."""
    nfft, per, nrows, sigma, d, S = 1024, 8, 400, 0.05, 0.01, 400.0
    b = 200
    plat = [(b, tone_amplitude(nfft, sigma, S), [(100, 2), (300, 2)])]
    assert sum(r for _, r in plat[0][2]) / nrows == d
    x = gated(np.random.default_rng(33), nfft, per, nrows, 0, sigma, plat)
    P, car = pdt.host_survey(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft)
    W, _, counts, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per)
    floor = float(np.median(P.astype(np.float64)))
    on_db = 10 * np.log10(W[[100, 101, 300, 301], b].astype(np.float64) / (floor * per))
    avg_db = 10 * np.log10(float(P[b]) / floor)
    print(f"d {d} S {S}: rows {on_db} dB over the floor while on, the average {avg_db:.2f} dB")
    assert np.all(on_db >= 15.0 + 6.0) and avg_db <= 15.0 - 4.0
    assert car == []
    assert [(f.first_row, f.rows) for f in found] == [(100, 2), (300, 2)]
    for f in found:
        assert abs(f.offset_hz - b * IN_RATE / nfft) <= IN_RATE / nfft and f.peak_db >= 21.0
        assert f.floor_power == np.float32(floor)
    assert counts.sum() == 4


def test_constant_tone_and_max_s(pdt):
    """A line that is always there (offset 0: a receiver's DC spike) beside a platform's bursts: with max_s shorter than the capture
    the line is gone and the bursts remain; without it the line is one burst as long as the stretch."""
    nfft, per, nrows, sigma = 1024, 8, 60, 0.05
    row_s = per * nfft / IN_RATE
    amp = tone_amplitude(nfft, sigma, 1000.0)
    plat = [(0, amp, [(0, nrows + 1)]), (300, amp, [(10, 5), (40, 7)])]
    x = gated(np.random.default_rng(44), nfft, per, nrows, 100, sigma, plat)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per, max_s=20 * row_s)
    assert [(f.first_row, f.rows) for f in found] == [(10, 5), (40, 7)]
    assert all(abs(f.offset_hz - 300 * IN_RATE / nfft) <= IN_RATE / nfft for f in found)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per)
    assert [(f.first_row, f.rows) for f in found] == [(0, nrows), (10, 5), (40, 7)]
    assert abs(found[0].offset_hz) <= IN_RATE / nfft and found[0].duration_s == nrows * per * nfft / IN_RATE
    car = pdt.burst_carriers(found, ARGOS_RANGE)
    assert sorted(round(c.offset_hz * nfft / IN_RATE) for c in car) == [0, 300]


def test_a_peak_beside_a_much_stronger_one_in_its_row_is_not_linked(pdt):
    """The sideband rule of the linking (csrc/pdt_bursts.h): guard_hz = 15 625 Hz is 16 bins here, so the rule reaches 64 bins.  A
    platform 55 dB over the floor in rows 10 .. 19 at bin 300; tones 22 dB over the floor, 33 dB weaker: at bin 330 in rows 12 .. 17
    (outside the guard, inside the rule's reach, at the same time: dropped), at bin 330 in rows 30 .. 35 (another time: kept), at bin
    400 in rows 10 .. 19 (100 bins away: kept).  The rows' peak records keep all of them."""
    nfft, per, nrows, sigma = 1024, 8, 40, 0.01
    strong, weak = tone_amplitude(nfft, sigma, 10 ** 5.5), tone_amplitude(nfft, sigma, 10 ** 2.2)
    plat = [(300, strong, [(10, 10)]), (330, weak, [(12, 6), (30, 6)]), (400, weak, [(10, 10)])]
    x = gated(np.random.default_rng(55), nfft, per, nrows, 0, sigma, plat)
    _, peaks, counts, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per)
    assert sorted(peaks["bin"][14][: counts[14]]) == [300, 330, 400]
    got = [(f.first_row, f.rows, round(f.offset_hz * nfft / IN_RATE)) for f in found]
    assert got == [(10, 10, 300), (10, 10, 400), (30, 6, 330)]
    assert len(pdt.burst_carriers(found, ARGOS_RANGE)) == 3


def test_a_strong_constant_line_does_not_hide_a_distant_platform(pdt):
    """A line that is always there, 45 dB over the floor at offset 0, and a platform 200 kHz away whose two-row bursts stand 19 dB
    over the floor, 26 dB weaker: the platform is a platform with max_s (the line is gone) and without it (the line is one more)."""
    nfft, per, nrows, sigma = 1024, 8, 400, 0.01
    plat = [(0, tone_amplitude(nfft, sigma, 10 ** 4.5), [(0, nrows)]), (205, tone_amplitude(nfft, sigma, 10 ** 1.9), [(100, 2), (300, 2)])]
    x = gated(np.random.default_rng(66), nfft, per, nrows, 0, sigma, plat)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per)
    assert [(f.first_row, f.rows) for f in found] == [(0, nrows), (100, 2), (300, 2)]
    assert found[0].peak_db - max(f.peak_db for f in found[1:]) >= 25.0
    car = pdt.burst_carriers(found, ARGOS_RANGE)
    assert [round(c.offset_hz * nfft / IN_RATE) for c in car] == [0, 205]
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per, max_s=5 * per * nfft / IN_RATE)
    assert [(f.first_row, f.rows) for f in found] == [(100, 2), (300, 2)]
    assert [round(c.offset_hz * nfft / IN_RATE) for c in pdt.burst_carriers(found, ARGOS_RANGE)] == [205]


def test_noise_only(pdt):
    """Gaussian noise, fixed seed, R = 1, 10240 rows of 1024 bins (about 10^7 cells): a cell is exponential, 31.6 times its mean is
    passed with probability 2 10^-14 -- no row has a peak, no burst."""
    nfft, nrows = 1024, 10240
    rng = np.random.default_rng(5)
    x = np.round(rng.standard_normal((nrows * nfft, 2)) * 3000.0).astype(np.int16)
    _, _, counts, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, rows=False, nfft=nfft, rows_per=1)
    assert len(counts) == nrows and counts.sum() == 0 and found == []


def test_arguments(pdt):
    x = np.zeros((2 * 8 * 4096, 2), dtype=np.int16)
    assert pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x)[3] == []           # the defaults: nfft 4096, R 8, two rows
    for bad in (dict(nfft=2048), dict(rows_per=65), dict(rows_per=-1), dict(cap=0), dict(gap_rows=-1), dict(first_frame=len(x) + 1)):
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, **bad)
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x[: 8 * 4096 - 1])       # shorter than one row
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        pdt.burst_carriers([], ARGOS_RANGE, cap=0)
    assert pdt.burst_carriers([], ARGOS_RANGE) == []
