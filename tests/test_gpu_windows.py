"""Every burst of a wideband capture in a window of its own, on the GPU: the kernel over a table of windows against the host restatement
bit for bit, each window against the single call it stands for, the payloads sent against the payloads decoded -- the first burst
of every platform and a platform that drifts through the loop's range included --, states and arguments, and `-t each` on the
command line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_bursts import STAT_FIELDS
from test_gpu_channel_input import fmt_code, random_capture
from test_windows import ARGOS_RANGE, D, FS, IN_RATE, OFFSETS, PERIOD_S, RESIDUAL, SEEDS, expected_payload, platforms, to_cu8

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
FORMATS = ("pcm16", "f32", "cu8", "cs8")


def resident(x: np.ndarray):
    dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return dev


def pool(pdt, mode: int, fs: int, decim: int, n: int):
    return [pdt.Demodulator(mode, fs).set_channel(decim, 0.0) for _ in range(n)]


def close_all(ds):
    for d in ds:
        d.close()


def check_against_host_ddc(pdt, ds, x, in_rate, decim, windows):
    for i, (d, w) in enumerate(zip(ds, windows)):
        want = pdt.host_ddc(in_rate, decim, w.offset_hz, x[w.first_frame: w.first_frame + w.nframes])
        assert d.stage_len(pdt.ST_CHANNEL) == (w.nframes + decim - 1) // decim, (i, w)
        got = d.stage(pdt.ST_CHANNEL).tobytes() if w.nframes else b""
        assert got == want.tobytes(), (i, w)
        assert d.stats().samples == (w.nframes + decim - 1) // decim


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("decim", (2, 4, 7, 16, 64))
def test_kernel_equals_host_restatement(pdt, decim, fmt):
    """PDT_ST_CHANNEL of every context is pdt_host_ddc of its slice at its offset, bit for bit, for windows of one call that start at
    frame 0, end at the last frame, are 1 frame, less than the filter's half-span, exactly one tile and one tile + 1 long, begin at an
    odd frame (an unsigned 8-bit window is then 2-byte aligned only) and at a 16-byte boundary with tiles inside them (the wide
    loads), overlap, repeat at another offset, and are empty."""
    rng = np.random.default_rng(7000 + 10 * decim + FORMATS.index(fmt))
    fs, n = 250000, 40000
    in_rate = fs * decim
    tile = 2048 // decim * decim
    x = random_capture(rng, fmt, n)
    W = pdt.Window
    windows = [W(0, 3001, 0.31 * in_rate), W(n - 2500, 2500, -0.123456 * in_rate), W(123, 1, 1000.0), W(5001, 8 * decim - 1, -77777.0),
               W(1000, tile, 0.2 * in_rate), W(2002, tile + 1, -0.2 * in_rate), W(777, 3 * tile + 5, 0.4 * in_rate),
               W(4096, 3 * tile + 77, -0.45 * in_rate), W(10000, 5000, 12345.0), W(12000, 5000, -54321.0),
               W(20000, 4321, 0.05 * in_rate), W(20000, 4321, -0.37 * in_rate), W(30000, 0, 5000.0)]
    dev = resident(x)
    ds = pool(pdt, pdt.MODE_POES, fs, decim, len(windows))
    try:
        pdt.demod_windows(ds, dev.data_ptr(), n, fmt_code(pdt, x), windows)
        check_against_host_ddc(pdt, ds, x, in_rate, decim, windows)
    finally:
        close_all(ds)


def test_forty_windows_of_unequal_length(pdt):
    """40 windows of 300 .. 3 000 frames at decimation 4: one launch, tiles of many windows, most of them edge tiles."""
    rng = np.random.default_rng(4040)
    fs, decim, n = 250000, 4, 40000
    in_rate = fs * decim
    x = random_capture(rng, "pcm16", n)
    windows = []
    for i in range(40):
        length = int(rng.integers(300, 3001))
        windows.append(pdt.Window(int(rng.integers(0, n - length + 1)), length, float(rng.uniform(-0.49, 0.49) * in_rate)))
    dev = resident(x)
    ds = pool(pdt, pdt.MODE_POES, fs, decim, len(windows))
    try:
        pdt.demod_windows(ds, dev.data_ptr(), n, pdt.FMT_WB_PCM16, windows)
        check_against_host_ddc(pdt, ds, x, in_rate, decim, windows)
    finally:
        close_all(ds)


@pytest.fixture(scope="module")
def argos_pair(pdt):
    """The two synthetic ARGOS platforms of tests/test_gpu_bursts.py, 15 s; its unsigned 8-bit rendering; the bursts of both."""
    x, params = platforms(pdt, IN_RATE, 15.0, OFFSETS, SEEDS, RESIDUAL)
    return x, to_cu8(x), params


def held(pdt, d):
    """what a context holds after a call: text, frame records, PDT_ST_CHANNEL, the statistics that describe the capture"""
    st = d.stats()
    chan = d.stage(pdt.ST_CHANNEL).tobytes() if d.stage_len(pdt.ST_CHANNEL) else b""
    return d.text(), d.frames_array().tobytes(), chan, tuple(getattr(st, f) for f in STAT_FIELDS)


def test_each_window_equals_the_single_call(pdt, argos_pair):
    """Through the device entry, the host entry and the held entry, twice on the same contexts: text, frames, PDT_ST_CHANNEL and the
    statistics of every context are what a fresh context gets from set_channel + demod_device_channel on the slice."""
    x = argos_pair[0][: 6 * IN_RATE]
    dev = resident(x)
    fmt = fmt_code(pdt, x)
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        found = holder.bursts(x)
        windows = pdt.burst_windows(found, IN_RATE, len(x))
        assert len(windows) == 8 and all(w.nframes > 0.3 * IN_RATE for w in windows)
        alone = []
        for w in windows:
            with pdt.Demodulator(pdt.MODE_ARGOS, FS) as d:
                d.set_channel(D, w.offset_hz).demod_device_channel(dev.data_ptr() + w.first_frame * 2 * x.itemsize, w.nframes, fmt)
                alone.append(held(pdt, d))
        assert sum(len(a[0]) > 0 for a in alone) >= 6                     # (this is about frames, not about empty results)
        ds = pool(pdt, pdt.MODE_ARGOS, FS, D, len(windows))
        try:
            for rep in range(2):
                pdt.demod_windows(ds, dev.data_ptr(), len(x), fmt, windows)
                assert [held(pdt, d) for d in ds] == alone, ("device", rep)
                pdt.demod_windows(ds, x, 0, 0, windows)
                assert [held(pdt, d) for d in ds] == alone, ("host", rep)
                holder.demod_windows_held(ds, windows)
                assert [held(pdt, d) for d in ds] == alone, ("held", rep)
        finally:
            close_all(ds)


@pytest.mark.parametrize("rendering", ("int16", "cu8"))
def test_decodes_what_was_sent_the_first_burst_included(pdt, argos_pair, rendering):
    """The 15 s capture: at least 18 of the 20 windows yield their burst's payload, and no window yields a payload that was not
    sent.  The host pipeline (tests/test_windows.py) decodes 20 of 20; the two bursts of margin allow for the device's portable
    double sincos against libm's."""
    x = argos_pair[0] if rendering == "int16" else argos_pair[1]
    params = argos_pair[2]
    nb = int(len(x) / IN_RATE / PERIOD_S)
    sent = {bytes(pdt.synth_argos_payload(p, b)) for p in params for b in range(nb)}
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        found = holder.bursts(x)
        windows = pdt.burst_windows(found, IN_RATE, len(x))
        assert len(windows) == 20
        ds = pool(pdt, pdt.MODE_ARGOS, FS, D, len(windows))
        try:
            holder.demod_windows_held(ds, windows)
            hit, extra, first = 0, 0, 0
            for d, w in zip(ds, windows):
                got = [bytes(f["bytes"][:7]) for f in d.frames_array() if f["complete"]]
                ok = expected_payload(pdt, params, OFFSETS, RESIDUAL, w, IN_RATE) in got
                hit += ok
                first += ok and w.first_frame < IN_RATE
                extra += sum(g not in sent for g in got)
        finally:
            close_all(ds)
    print(rendering, "windows with their payload:", hit, "of", len(windows), "first bursts:", first, "payloads not sent:", extra)
    assert hit >= 18 and extra == 0


def test_a_drifting_platform(pdt):
    """One platform whose carrier ramps from +1200 to -1200 Hz about its centre over a pass: per-burst windows decode at least 12
    of its 14 bursts (the host pipeline: 14), the whole capture at the platform's mean offset fewer than 7 (the host: 2) -- the
    ARGOS loop sweeps +-550 Hz."""
    secs, centre = 24.0, 250000.0
    n = int(secs * IN_RATE)
    p = pdt.synth_params(1, IN_RATE, centre, 8)
    p.amplitude //= 2
    p.noise_gain //= 2
    pdt.synth_lib().pdt_synth_set_pass(C.byref(p), 2 * IN_RATE, 23 * IN_RATE, centre + 1200.0, centre - 1200.0, 0.0)
    x = np.zeros((n, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, x.ctypes.data)
    sent = {bytes(pdt.synth_argos_payload(p, b)) for b in range(2, 16)}    # the bursts at 3.0, 4.5 .. 22.5 s lie inside the pass
    assert len(sent) == 14
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        found = holder.bursts(x)
        windows = pdt.burst_windows(found, IN_RATE, len(x))
        ds = pool(pdt, pdt.MODE_ARGOS, FS, D, len(windows))
        try:
            holder.demod_windows_held(ds, windows)
            each = {bytes(f["bytes"][:7]) for d in ds for f in d.frames_array() if f["complete"]}
        finally:
            close_all(ds)
        car = pdt.burst_carriers(found, ARGOS_RANGE)
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, c.offset_hz) for c in car]
        try:
            pdt.demod_channels(ds, x)
            whole = {bytes(f["bytes"][:7]) for d in ds for f in d.frames_array() if f["complete"]}
        finally:
            close_all(ds)
    print("bursts found:", len(found), "platforms:", len(car), "decoded per burst:", len(each & sent), "whole capture:", len(whole & sent))
    assert len(each & sent) >= 12 and each <= sent
    assert len(whole & sent) < 7


def test_state_and_arguments(pdt, argos_pair):
    x = argos_pair[0][: 2 * IN_RATE]
    dev = resident(x)
    fmt = fmt_code(pdt, x)
    W = pdt.Window
    good = [W(1000, 50000, 250120.0), W(60001, 40000, -333180.0)]
    ds = pool(pdt, pdt.MODE_ARGOS, FS, D, 2)
    other = pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D // 2, 0.0)         # another decimation
    fresh = pdt.Demodulator(pdt.MODE_ARGOS, FS)
    holder = pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, 0.0)
    try:
        pdt.demod_windows(ds, dev.data_ptr(), len(x), fmt, good)
        want = [d.stage(pdt.ST_CHANNEL).tobytes() for d in ds]
        for bad in ([good[0], W(len(x) - 10, 11, 0.0)], [good[0], W(len(x) + 1, 1, 0.0)], [W(0, len(x) + 1, 0.0), good[1]],
                    [good[0], W(0, 100, 0.5 * IN_RATE)], [good[0], W(0, 100, -0.5 * IN_RATE)], [good[0], W(0, 100, float("nan"))]):
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                pdt.demod_windows(ds, dev.data_ptr(), len(x), fmt, bad)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.demod_windows([ds[0], other], dev.data_ptr(), len(x), fmt, good)          # mixed decimations
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.demod_windows([ds[0], ds[0]], dev.data_ptr(), len(x), fmt, good)          # a context given twice
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.demod_windows(ds, dev.data_ptr(), len(x), pdt.FMT_PCM16, good)            # not a wideband format
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            pdt.demod_windows([ds[0], fresh], dev.data_ptr(), len(x), fmt, good)          # no set_channel
        ds[1].stream_push_channel(x[:4096])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            pdt.demod_windows(ds, dev.data_ptr(), len(x), fmt, good)                      # an open stream
        ds[1].stream_end()
        # a refused call changed nothing: offsets are where the last good call left them, and the call repeats
        pdt.demod_windows(ds, dev.data_ptr(), len(x), fmt, good)
        assert [d.stage(pdt.ST_CHANNEL).tobytes() for d in ds] == want
        pdt.demod_windows([], dev.data_ptr(), len(x), fmt, [])
        # the held capture
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            holder.demod_windows_held(ds, good)                                           # before any search
        holder.survey(x, nfft=4096)
        spec = holder.survey_spectrum().tobytes()
        holder.demod_windows_held(ds, good)                                               # a survey holds the capture too
        assert [d.stage(pdt.ST_CHANNEL).tobytes() for d in ds] == want
        found = holder.bursts(x)
        nrows = holder.bursts_shape()[2]
        rows, peaks = holder.waterfall_rows(0, nrows).tobytes(), [a.tobytes() for a in holder.burst_peaks(0, nrows)]
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            holder.demod_windows_held([ds[0], holder], good)                              # the holder among the contexts
        holder.demod_windows_held(ds, good)
        assert [d.stage(pdt.ST_CHANNEL).tobytes() for d in ds] == want
        assert holder.waterfall_rows(0, nrows).tobytes() == rows and [a.tobytes() for a in holder.burst_peaks(0, nrows)] == peaks
        assert holder.survey_spectrum().tobytes() == spec and holder.bursts(x) == found
        assert len(holder.frames_array()) == 0 and holder.stage_len(pdt.ST_CHANNEL) == 0
        holder.demod_channel(x)                                                           # the holder's buffer takes another capture
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            holder.demod_windows_held(ds, good)
        # ... and so it does in the stage hooks that put their samples there: a few samples that fit the buffer as it is (the
        # capture's bytes would be the hook's), and more than it holds (the buffer moves)
        for search in (lambda: holder.bursts(x), lambda: holder.survey(x, nfft=4096)):
            for hook, n in ((holder.stage_static_gain, 5000), (holder.stage_pll, 5000), (holder.stage_static_gain, len(x) + 100000)):
                search()
                holder.demod_windows_held(ds, good)
                assert [d.stage(pdt.ST_CHANNEL).tobytes() for d in ds] == want
                hook(np.zeros((n, 2), dtype=np.int16))
                with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
                    holder.demod_windows_held(ds, good)
        holder.bursts(x)
        holder.stage_pll(x[:5000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            holder.waterfall_rows(0, 1)
    finally:
        close_all(ds + [other, fresh, holder])


def test_command_line_each(pdt, argos_pair, tmp_path):
    x8, params = argos_pair[1], argos_pair[2]
    cu8 = str(tmp_path / "capture.cu8")
    x8.tofile(cu8)
    exe = os.path.join(BIN, "demodARGOS")
    out = str(tmp_path / "out")
    base = [exe, "-x", str(D), "-s", str(IN_RATE // 1000)]
    r = subprocess.run(base + ["-t", "each", "-o", out, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert len(re.findall(r"^Burst at ([0-9.]+) s, ([0-9.]+) s long, ([+-][0-9.]+) Khz, ([0-9.]+) dB over the floor$", r.stdout, flags=re.M)) == 20
    lines = re.findall(r"^Burst (\d+): lock ([+-][0-9.]+ Hz|none), (\d+) packets$", r.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == list(range(20))
    summary = re.findall(r"^Bursts: (\d+), locked: (\d+), packets: (\d+)$", r.stdout, flags=re.M)
    assert summary == [("20", str(sum(l[1] != "none" for l in lines)), str(sum(int(l[2]) for l in lines)))]
    # the file: the windows' records from the binding, each time counted from the capture's start
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x8, max_s=5.0), IN_RATE, len(x8))
        ds = pool(pdt, pdt.MODE_ARGOS, FS, D, len(windows))
        try:
            holder.demod_windows_held(ds, windows)
            parts = []
            for d, w, l in zip(ds, windows, lines):
                fr = d.frames_array().copy()
                fr["time"] += w.first_frame / IN_RATE
                parts.append(fr)
                assert int(l[2]) == len(fr)
        finally:
            close_all(ds)
    text = open(out, "rb").read()
    assert text == pdt.format_frames(np.concatenate(parts)) and len(text) > 500
    # a pool of 8 contexts: three rounds, the contexts used again with other windows -- the same lines and the same file
    out8 = str(tmp_path / "out8")
    r8 = subprocess.run(base + ["-t", "each:8", "-o", out8, cu8], capture_output=True, text=True, timeout=300)
    assert r8.returncode == 0, r8.stdout[-2000:]
    assert re.findall(r"^Burst (\d+): lock ([+-][0-9.]+ Hz|none), (\d+) packets$", r8.stdout, flags=re.M) == lines
    assert open(out8, "rb").read() == text
    for bad in ("each:0", "each:65", "eachother"):
        rb = subprocess.run(base + ["-t", bad, "-o", out8 + "x", cu8], capture_output=True, text=True, timeout=300)
        assert rb.returncode == 1 and "-t each or -t each:N" in rb.stdout and not os.path.exists(out8 + "x")
    # noise: the message, no file, exit status 1
    p = pdt.synth_params(1, IN_RATE, 1000.0, 5)
    p.amplitude = 0
    noise = np.zeros((2000000, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, len(noise), noise.ctypes.data)
    ncu8 = str(tmp_path / "noise.cu8")
    to_cu8(noise).tofile(ncu8)
    nout = str(tmp_path / "noise.txt")
    r = subprocess.run(base + ["-t", "each", "-o", nout, ncu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and re.search(r"^No burst found$", r.stdout, flags=re.M)
    assert not any(f.startswith("noise.txt") for f in os.listdir(tmp_path))
    r = subprocess.run(base + ["-t", "each", "-t", "250", "-o", nout, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot be combined" in r.stdout and not os.path.exists(nout)
    # -t bursts is what it was: the platforms, a file each, the frames of contexts given the printed offsets
    bout = str(tmp_path / "bursts.txt")
    r = subprocess.run(base + ["-t", "bursts", "-o", bout, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "Burst 0:" not in r.stdout and "Bursts:" not in r.stdout
    chans = re.findall(r"^Channel (\d+) at ([+-][0-9.]+) Khz \(found, ([0-9.]+) dB over the floor\)$", r.stdout, flags=re.M)
    assert [int(c[0]) for c in chans] == [0, 1]
    ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, float(c[1]) * 1000.0) for c in chans]
    try:
        pdt.demod_channels(ds, x8)
        for i, d in enumerate(ds):
            assert open(f"{bout}.{i}", "rb").read() == d.text() and len(d.text()) > 100
    finally:
        close_all(ds)
