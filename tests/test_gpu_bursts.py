"""The burst search on the GPU: the waterfall's rows (k_spectra), k_row_peaks' peaks and the burst list against the host restatement
bit for bit, captures off their pair boundary, a slab seam, that a burst search leaves no trace in a context, bursts ->
burst_carriers -> set_channel -> demod_channels on two synthetic ARGOS platforms, and `-t bursts` on the command line."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_bursts import ARGOS_RANGE, gated, tone_amplitude
from test_gpu_channel_input import carriers, fmt_code, to_cu8

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
FORMATS = ("pcm16", "f32", "cu8", "cs8")
IN_RATE, FS, D = 1000000, 31250, 32


def render(z: np.ndarray, fmt: str) -> np.ndarray:
    f = np.stack([z.real, z.imag], axis=1)
    if fmt == "f32":
        return f.astype(np.float32)
    if fmt == "pcm16":
        return np.round(f * 32767.0).astype(np.int16)
    if fmt == "cu8":
        return np.clip(np.round(f * 128.0 + 127.5), 0, 255).astype(np.uint8)
    return np.clip(np.round(f * 128.0), -128, 127).astype(np.int8)


def five_rows(rng, nfft: int, per: int, extra: int) -> np.ndarray:
    """Five rows and `extra` samples: silence; ten tones on bin centres, far enough apart to be ten lines (more than a row records);
    one full-scale impulse in the middle of every segment -- each of its transforms has the same power in EVERY bin, so the row is
    one N-fold tie, broken towards the lowest bin, and more than eight bins stand over the level --; the tones again in weak noise;
    silence."""
    row = per * nfft
    n = np.arange(row)
    tones = sum(0.08 * np.exp(2j * np.pi * b * n / nfft) for b in (5, 40, 90, 200, nfft // 2 - 3, nfft // 2 + 9, nfft - 300, nfft - 77, nfft - 30, nfft - 2))
    z = np.zeros(5 * row + extra, dtype=np.complex128)
    z[row: 2 * row] = tones
    z[2 * row + nfft // 2: 3 * row: nfft] = 0.99
    z[3 * row: 4 * row] = tones + 0.01 * (rng.standard_normal(row) + 1j * rng.standard_normal(row))
    return z


def same_search(pdt, d, x, dev=None, **cfg):
    """One burst search on the context (from host memory, or resident at address dev) against the hook's: rows, peaks, bursts."""
    rows, peaks, counts, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, **cfg)
    got = d.bursts(x, **cfg) if dev is None else d.bursts_device(dev, len(x), fmt_code(pdt, x), **cfg)
    assert got == found
    gp, gc = d.burst_peaks(0, len(rows))
    assert np.array_equal(gc, counts) and gp.tobytes() == peaks.tobytes()
    assert d.waterfall_rows(0, len(rows)).tobytes() == rows.tobytes()
    assert d.bursts_shape() == (rows.shape[1], int(cfg.get("rows_per", 8)), len(rows))
    return rows, peaks, counts, found


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nfft", (1024, 4096, 16384))
def test_kernels_equal_host_restatement(pdt, nfft, fmt):
    """Rows (pdt_waterfall_rows), per-row peaks and the burst list are pdt_host_bursts', bit for bit, at R = 1, 3, 8 and 64; the
    capture ends with an incomplete row and an incomplete segment.  Row 1 has ten lines (the cap of eight is hit), row 2 is a tie
    of every bin.  threshold_db 3: the floor is the median of the average over five rows, one of which is flat.  At N = 1024 also
    noise with one gated tone over several workgroups of several rows, the last workgroup short: R = 3, 47 rows (21 a workgroup) and
    two segments and 11 samples, and R = 1, 130 rows (64 a workgroup) and 11 samples."""
    rng = np.random.default_rng(nfft + FORMATS.index(fmt))
    guard = 3.5 * IN_RATE / nfft
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as d:
        d.set_channel(D, 0.0)
        for per in (1, 3, 8, 64):
            x = render(five_rows(rng, nfft, per, (per - 1) * nfft + 11 if per > 1 else 11), fmt)
            rows, peaks, counts, found = same_search(pdt, d, x, nfft=nfft, rows_per=per, threshold_db=3.0, guard_hz=guard, merge_hz=guard)
            assert len(rows) == 5 and counts[1] == 8 and counts[2] == 8, counts
            if fmt != "cu8":                                               # (unsigned 8-bit has no zero: its flat row is flat to a few ulp only)
                assert np.all(rows[2] == rows[2][0]) and counts[0] == 0 and counts[4] == 0
                assert list(peaks["bin"][2]) == [4 * k for k in range(8)]  # guard: 3 bins each side
            assert len(found) >= 1
            # a stretch of it
            same = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, nfft=nfft, rows_per=per, threshold_db=3.0, guard_hz=guard, first_frame=per * nfft - 5,
                                   nframes=3 * per * nfft + 9)
            assert d.bursts(x, nfft=nfft, rows_per=per, threshold_db=3.0, guard_hz=guard, first_frame=per * nfft - 5, nframes=3 * per * nfft + 9) == same[3]
            assert d.waterfall_rows(1, 2).tobytes() == same[0][1:3].tobytes()
        if nfft == 1024:
            # several workgroups of several rows, the last one short: R = 3 gives a workgroup 21 rows, R = 1 gives it 64
            for per, nrows, extra in ((3, 47, 2 * nfft + 11), (1, 130, 11)):
                tone = [(100, tone_amplitude(nfft, 0.05, 1000.0), [(nrows // 3, nrows // 4)])]
                z = gated(rng, nfft, per, nrows, extra, 0.05, tone)
                x = render(z[:, 0].astype(np.float64) + 1j * z[:, 1], fmt)
                rows, _, counts, found = same_search(pdt, d, x, nfft=nfft, rows_per=per)
                assert len(rows) == nrows and counts.sum() >= nrows // 4 and len(found) >= 1
                for first in (20, 63):                                     # three rows across the first workgroup's last row
                    if first + 3 <= nrows:
                        assert d.waterfall_rows(first, 3).tobytes() == rows[first: first + 3].tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
def test_capture_aligned_to_its_element_but_not_to_its_pair(pdt, fmt):
    """A resident capture that begins half a sample off a pair boundary, and 0, 1 and 3 whole samples further on: every segment is
    loaded sample by sample, and rows, peaks and bursts are the hook's of the same bytes."""
    rng = np.random.default_rng(900 + FORMATS.index(fmt))
    nfft, per = 1024, 3
    n = 5 * per * nfft + 9
    flat = render(five_rows(rng, nfft, per, 9 + 4), fmt).reshape(-1)
    dev = torch.from_numpy(flat.view(np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as d:
        d.set_channel(D, 0.0)
        for skip in (0, 1, 3):
            first = 2 * skip + 1
            host = flat[first: first + 2 * n].reshape(n, 2)
            same_search(pdt, d, host, dev=dev.data_ptr() + first * flat.itemsize, nfft=nfft, rows_per=per, threshold_db=3.0)


def test_slab_seam(pdt, monkeypatch):
    """Slabs of two rows (the developer switch PDT_BURST_SLAB_ROWS): a burst over rows 1 .. 4 spans two seams, and rows, peaks and
    bursts are those of the one-slab search and of the hook."""
    nfft, per, nrows = 1024, 8, 7
    x = gated(np.random.default_rng(3), nfft, per, nrows, 100, 0.05, [(100, tone_amplitude(nfft, 0.05, 1000.0), [(1, 4)])])
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as d:
        d.set_channel(D, 0.0)
        one = same_search(pdt, d, x, nfft=nfft, rows_per=per)
    assert [(f.first_row, f.rows) for f in one[3]] == [(1, 4)]
    monkeypatch.setenv("PDT_BURST_SLAB_ROWS", "2")
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as d:
        d.set_channel(D, 0.0)
        two = same_search(pdt, d, x, nfft=nfft, rows_per=per)
        assert d.waterfall_rows(1, 5).tobytes() == one[0][1:6].tobytes()
    assert two[3] == one[3]


STAT_FIELDS = ("samples", "out_samples", "symbols", "bits", "frames", "lock_sample", "lock_freq_hz", "norm_factor", "avg_phase")


@pytest.fixture(scope="module")
def argos_pair(pdt):
    """Two synthetic ARGOS platforms in one wideband capture (the helpers of tests/test_gpu_channel_input.py, their amplitudes)."""
    in_rate, secs = 1024000, 15.0
    offsets = (250000.0, -333300.0)
    x, params = carriers(pdt, 1, in_rate, secs, offsets, (8, 9), 120.0)
    return in_rate, offsets, x, params


def sent_and_got(pdt, p, d, n, in_rate, decim):
    period = in_rate * 3 // 2
    nb = int(n // period)
    st = d.stats()
    sent = [bytes(pdt.synth_argos_payload(p, b)) for b in range(nb)]
    got = [bytes(f["bytes"][:7]) for f in d.frames_array() if f["complete"]]
    after = [sent[b] for b in range(nb) if b * period >= st.lock_sample * decim]
    return st, sent, got, after


def test_search_leaves_no_trace(pdt, argos_pair):
    """survey, burst search, demodulation on one context: the survey's spectrum, the frames and the statistics are what they are
    without the burst search."""
    in_rate, offsets, x, _ = argos_pair
    fs = in_rate // D
    out = []
    for with_search in (False, True):
        with pdt.Demodulator(pdt.MODE_ARGOS, fs) as d:
            d.set_channel(D, offsets[0])
            car = d.survey(x, nfft=4096)
            spec = d.survey_spectrum().tobytes()
            if with_search:
                assert len(d.bursts(x)) >= 2
                assert d.survey_spectrum().tobytes() == spec
                assert len(d.frames_array()) == 0 and d.stage_len(pdt.ST_CHANNEL) == 0
            d.demod_channel(x)
            if with_search:                                                # the input buffer the search read has taken another capture
                with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
                    d.waterfall_rows(0, 1)
            st = d.stats()
            out.append((car, spec, d.frames_array().tobytes(), d.text(), tuple(getattr(st, f) for f in STAT_FIELDS), d.survey(x, nfft=4096)))
    assert out[0] == out[1] and len(out[0][2]) > 0


def test_bursts_then_demodulate(pdt, argos_pair):
    in_rate, offsets, x, params = argos_pair
    fs = in_rate // D
    dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    fmt = fmt_code(pdt, x)
    ds = [pdt.Demodulator(pdt.MODE_ARGOS, fs).set_channel(D, 0.0) for _ in offsets]
    try:
        found = ds[0].bursts_device(dev.data_ptr(), len(x), fmt)
        assert len(found) >= 2 * 9                                        # ten bursts each in 15 s, one every 1.5 s
        car = pdt.burst_carriers(found, ARGOS_RANGE)
        assert len(car) == 2
        for d, c in zip(ds, car):
            d.set_channel(D, c.offset_hz)
        pdt.demod_channels(ds, dev.data_ptr(), len(x), fmt)
        for d, c in zip(ds, car):
            near = int(np.argmin([abs(c.offset_hz - (off + 120.0)) for off in offsets]))
            assert abs(c.offset_hz - (offsets[near] + 120.0)) <= in_rate / 4096
            st, sent, got, after = sent_and_got(pdt, params[near], d, len(x), in_rate, D)
            print(c, st.lock_sample, st.lock_freq_hz, len(got), len(after))
            assert st.lock_sample >= 0 and len(after) >= len(sent) // 2
            assert all(s in got for s in after) and all(g in sent for g in got)
    finally:
        for d in ds:
            d.close()


def test_command_line_bursts(pdt, argos_pair, tmp_path):
    in_rate, offsets, x, params = argos_pair
    cu8 = str(tmp_path / "capture.cu8")
    to_cu8(x).tofile(cu8)
    exe = os.path.join(BIN, "demodARGOS")
    out = str(tmp_path / "bursts.txt")
    r = subprocess.run([exe, "-x", str(D), "-s", str(in_rate / 1000.0), "-t", "bursts", "-o", out, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    bursts = re.findall(r"^Burst at ([0-9.]+) s, ([0-9.]+) s long, ([+-][0-9.]+) Khz, ([0-9.]+) dB over the floor$", r.stdout, flags=re.M)
    assert len(bursts) >= 2 * 9
    lines = re.findall(r"^Channel (\d+) at ([+-][0-9.]+) Khz \(found, ([0-9.]+) dB over the floor\)$", r.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == [0, 1]
    assert sorted(round(float(l[1])) for l in lines) == [-333, 250]
    # the two files are what contexts given the printed offsets hold, and those are the payloads sent
    fs = in_rate // D
    ds = [pdt.Demodulator(pdt.MODE_ARGOS, fs).set_channel(D, float(l[1]) * 1000.0) for l in lines]
    try:
        x8 = to_cu8(x)
        pdt.demod_channels(ds, x8, len(x8), fmt_code(pdt, x8))
        for i, (d, l) in enumerate(zip(ds, lines)):
            near = int(np.argmin([abs(float(l[1]) * 1000.0 - off) for off in offsets]))
            st, sent, got, after = sent_and_got(pdt, params[near], d, len(x), in_rate, D)
            assert st.lock_sample >= 0 and len(after) >= len(sent) // 2
            assert all(s in got for s in after) and all(g in sent for g in got)
            assert len(d.text()) > 100
    finally:
        for d in ds:
            d.close()
    num = str(tmp_path / "numbers.txt")
    r = subprocess.run([exe, "-x", str(D), "-s", str(in_rate / 1000.0), "-t", lines[0][1], "-t", lines[1][1], "-o", num, cu8], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    for i in (0, 1):
        a, b = open(f"{out}.{i}", "rb").read(), open(f"{num}.{i}", "rb").read()
        assert a == b and len(a) > 100
    # noise: the message, no file, exit status 1
    p = pdt.synth_params(1, in_rate, 1000.0, 5)
    p.amplitude = 0
    noise = np.zeros((2000000, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(pdt.C.byref(p), 0, len(noise), noise.ctypes.data)
    ncu8 = str(tmp_path / "noise.cu8")
    to_cu8(noise).tofile(ncu8)
    nout = str(tmp_path / "noise.txt")
    r = subprocess.run([exe, "-x", str(D), "-s", str(in_rate / 1000.0), "-t", "bursts", "-o", nout, ncu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and re.search(r"^No burst found$", r.stdout, flags=re.M)
    assert not any(f.startswith("noise.txt") for f in os.listdir(tmp_path))
    r = subprocess.run([exe, "-x", str(D), "-s", str(in_rate / 1000.0), "-t", "bursts", "-t", "200", "-o", nout, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot be combined" in r.stdout and not os.path.exists(nout)
    r = subprocess.run([exe, "-t", "bursts", "-o", nout, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "-t requires -x" in r.stdout
