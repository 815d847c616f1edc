"""The carrier of a channel stream as a measurement, on the GPU: the kernel against the host restatement bit for bit at
every NFFT, many contexts in one launch, a context left as it was, states and arguments, the drifting platform's Doppler curve
through `-t each`'s pool path, and -M on the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_bursts import STAT_FIELDS
from test_tones import ARGOS_FREQ_BOUND_HZ, ARGOS_RANGE, D, FS, IN_RATE, OFFSETS, RESIDUAL, SEEDS, bad_cfgs, drifting_capture, platforms, tone, truth_hz

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
NFFTS = (1024, 4096, 16384)
POES_FS, POES_D = 250000, 2                     # a POES context at 250 ksps fed a float capture at twice that: the channel stream is ceil(n / 2) pairs


def channel_of(pdt, d, x: np.ndarray, offset: float = 0.0) -> np.ndarray:
    """x through the context's down-converter: the channel stream the kernel reads, as the host reads it."""
    d.set_channel(POES_D, offset).demod_channel(x)
    return d.stage(pdt.ST_CHANNEL)


def same(pdt, d, y: np.ndarray, offset: float, **cfg):
    got, want = d.tones(**cfg), pdt.host_tones(POES_FS, offset, y, **cfg)
    assert len(got) == len(want) > 0, cfg
    assert got.tobytes() == want.tobytes(), (cfg, got, want)
    return got


@pytest.mark.parametrize("nfft", NFFTS)
def test_kernel_equals_hook_bit_for_bit(pdt, nfft):
    """Raw record and derived doubles, byte for byte, on channel streams of 3 N + 5 pairs made from random float pairs plus a tone:
    first = 0, first = 1 (8-byte but not 16-byte aligned: the head path of the load), stride N / 2 + 1 (overlapping segments at changing
    alignment), a peak in the negative half, a peak at bin 0, the widest search set with the widest noise band, a real stream (a
    mirrored tone pair: keys that are equal where the arithmetic is symmetric), and an all-zero stream (every key equal)."""
    rng = np.random.default_rng(900 + nfft)
    m = 3 * nfft + 5
    n = POES_D * m - 1                                                   # (ceil(n / 2) = m)
    wide = dict(nfft=nfft, search_hz=0.5 * POES_FS * (1 - 0.5 / nfft), noise_lo=1, noise_hi=nfft // 2 - 1)
    with pdt.Demodulator(pdt.MODE_POES, POES_FS) as d:
        # a tone 37.3 bins up: in the wideband capture it lies at offset + 37.3 Fs / N
        offset = 60000.0
        f = offset + 37.3 * POES_FS / nfft
        x = (rng.uniform(-1.0, 1.0, (n, 2)) + tone(n, f / (POES_D * POES_FS))).astype(np.float32)
        y = channel_of(pdt, d, x, offset)
        assert len(y) == m
        r = same(pdt, d, y, offset, nfft=nfft, search_hz=0.4 * POES_FS)
        assert len(r) == 3 and np.all(r["bin"] == 37) and np.all(r["valid"] == 1)
        assert len(same(pdt, d, y, offset, nfft=nfft, search_hz=0.4 * POES_FS, first=1)) == 3
        assert len(same(pdt, d, y, offset, nfft=nfft, search_hz=0.4 * POES_FS, stride=nfft // 2 + 1)) == 5
        assert len(same(pdt, d, y, offset, nfft=nfft, search_hz=0.4 * POES_FS, first=3, stride=7, count=4)) == 4
        r = same(pdt, d, y, offset, **wide)
        assert np.all(r["noise_bins"] == nfft - 2) and np.all(r["bin"] == 37)
        r = same(pdt, d, y, offset, nfft=nfft, search_hz=20 * POES_FS / nfft)             # the tone is outside: a noise bin wins
        assert np.all((r["bin"] <= 20) | (r["bin"] >= nfft - 20))
        # the negative half, and bin 0
        for k, want_bin in ((-(nfft // 8) - 0.45, nfft - nfft // 8), (0.2, 0)):
            x = (rng.uniform(-1.0, 1.0, (n, 2)) + tone(n, (offset + k * POES_FS / nfft) / (POES_D * POES_FS))).astype(np.float32)
            y = channel_of(pdt, d, x, offset)
            r = same(pdt, d, y, offset, nfft=nfft, search_hz=0.4 * POES_FS)
            assert np.all(r["bin"] == want_bin), (k, r["bin"])
            same(pdt, d, y, offset, nfft=nfft, search_hz=0.4 * POES_FS, first=1, stride=nfft + 1)
        # a real stream at offset 0: the two lines of cos are each other's mirror
        x = np.zeros((n, 2), dtype=np.float32)
        x[:, 0] = 0.3 * rng.uniform(-1.0, 1.0, n) + np.cos(2 * np.pi * 50 / (POES_D * nfft) * np.arange(n))
        y = channel_of(pdt, d, x, 0.0)
        assert np.all(y[:, 1] == 0.0)
        r = same(pdt, d, y, 0.0, nfft=nfft, search_hz=0.4 * POES_FS, count=1)
        up = pdt.host_tones(POES_FS, 0.0, y[:, :], nfft=nfft, search_hz=0.4 * POES_FS, count=1)[0]
        print(f"nfft {nfft}: real stream, peak at bin {r[0]['bin']} (lines at 50 and {nfft - 50}), power {up['peak']}")
        assert r[0]["bin"] in (50, nfft - 50)
        same(pdt, d, y, 0.0, **wide)
        # all zeros: every key is 0, the lowest bin, not valid
        y = channel_of(pdt, d, np.zeros((n, 2), dtype=np.float32), 0.0)
        r = same(pdt, d, y, 0.0, nfft=nfft, search_hz=0.4 * POES_FS)
        assert np.all(r["valid"] == 0) and np.all(r["bin"] == 0) and np.all(np.isnan(r["cn0_dbhz"]))


def test_one_launch_for_many_contexts(pdt):
    """pdt_tones_batch over three contexts whose streams have different lengths, one of them too short for a segment: what three
    pdt_tones calls give, and the profiled first context shows exactly one k_tones launch."""
    rng = np.random.default_rng(77)
    nfft = 16384                                                         # the default at 250 ksps
    lens = (3 * nfft + 5, nfft - 1, nfft + 100)
    ds = [pdt.Demodulator(pdt.MODE_POES, POES_FS, profile=(i == 0)) for i in range(3)]
    try:
        for i, (d, m) in enumerate(zip(ds, lens)):
            n = POES_D * m
            off = 40000.0 * (i + 1)
            x = (rng.uniform(-1.0, 1.0, (n, 2)) + tone(n, (off + (i - 1) * 700.3) / (POES_D * POES_FS))).astype(np.float32)
            assert len(channel_of(pdt, d, x, off)) == m
        got = pdt.tones_batch(ds, cap=8)
        kt = ds[0].kernel_times()
        assert kt["k_tones"][0] == 1 and len(kt) > 1, kt
        alone = [d.tones(cap=8) for d in ds]
        assert [len(g) for g in got] == [3, 0, 1]
        assert [g.tobytes() for g in got] == [a.tobytes() for a in alone]
        assert ds[0].kernel_times()["k_tones"][0] == 1
        for i, d in enumerate(ds):
            want = pdt.host_tones(POES_FS, 40000.0 * (i + 1), d.stage(pdt.ST_CHANNEL), search_hz=4500.0, cap=8)
            assert got[i].tobytes() == want.tobytes()                    # (the default search_hz of a POES context is its loop's 4500 Hz)
        # another order, a subset, and none at all
        back = pdt.tones_batch(ds[::-1], cap=8, stride=5000)
        assert [b.tobytes() for b in back[::-1]] == [d.tones(cap=8, stride=5000).tobytes() for d in ds]
        assert pdt.tones_batch([], cap=8) == []
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.tones_batch([ds[0], ds[0]], cap=8)                       # a context given twice
        with pdt.Demodulator(pdt.MODE_POES, 50000) as other:
            x = rng.uniform(-1.0, 1.0, (40000, 2)).astype(np.float32)
            other.set_channel(POES_D, 1000.0).demod_channel(x)
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                pdt.tones_batch([ds[0], other], cap=8)                   # another sample rate
    finally:
        for d in ds:
            d.close()


@pytest.fixture(scope="module")
def argos_short(pdt):
    return platforms(pdt, IN_RATE, 4.0, OFFSETS, SEEDS, RESIDUAL)[0]


def test_leaves_no_trace(pdt, argos_short):
    """Frames, text, every stage, the statistics, pdt_survey_spectrum and pdt_burst_peaks of a context are what they were."""
    x = argos_short
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as d:
        d.set_channel(D, OFFSETS[0] + RESIDUAL)
        d.demod_channel(x)
        d.survey(x, nfft=16384)
        assert len(d.bursts(x)) >= 2                                     # (last: its rows and peaks live as long as the input buffer keeps the capture)

        def state():
            st = d.stats()
            nrows = d.bursts_shape()[2]
            stages = [d.stage(s).tobytes() for s in range(pdt.ST_CHANNEL + 1) if d.stage_len(s)]
            return (d.frames_array().tobytes(), d.text(), tuple(getattr(st, f) for f in STAT_FIELDS), [d.stage_len(s) for s in range(pdt.ST_CHANNEL + 1)],
                    stages, d.survey_spectrum().tobytes(), [a.tobytes() for a in d.burst_peaks(0, nrows)])

        before = state()
        assert len(before[0]) > 0 and d.stage_len(pdt.ST_CHANNEL) == len(x) // D
        got = d.tones()                                                  # (N = 4096: the survey's tables of 16384 points are replaced)
        assert len(got) == len(x) // D // 4096
        assert got.tobytes() == pdt.host_tones(FS, OFFSETS[0] + RESIDUAL, d.stage(pdt.ST_CHANNEL), search_hz=ARGOS_RANGE).tobytes()
        assert state() == before
        d.tones(nfft=1024, stride=333, cap=5)
        assert state() == before
        assert d.survey(x, nfft=16384) is not None and d.survey_spectrum().tobytes() == before[5]


def test_states_and_arguments(pdt, argos_short):
    x = argos_short[: IN_RATE]
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tones()                                                    # a fresh context
        d.set_channel(D, OFFSETS[0])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tones()                                                    # a channel, but no capture yet
        d.demod_channel(x)
        want = d.tones()
        assert len(want) == len(x) // D // 4096
        for kw in bad_cfgs(FS):                                          # the cases of tests/test_tones.py, through a context
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                d.tones(**kw)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.tones_batch([d], nfft=2048)
        assert d.tones().tobytes() == want.tobytes()                     # a refused call changed nothing
        d.demod(np.random.default_rng(5).integers(-3000, 3000, (20000, 2)).astype(np.int16))
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tones()                                                    # after pdt_demod_pcm16: no channel stream
        d.demod_channel(x)
        assert d.tones().tobytes() == want.tobytes()
        d.stream_push_channel(x[:40000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tones()                                                    # a stream is open
        d.stream_end()
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tones()                                                    # ... and a stream that has ended left pieces, no channel stream
        d.demod_channel(x)
        assert d.tones().tobytes() == want.tobytes()
        assert len(d.tones(first=len(x) // D - 4095)) == 0               # less than a segment left


@pytest.fixture(scope="module")
def drifting(pdt):
    return drifting_capture(pdt)


def test_the_doppler_curve_of_a_drifting_platform(pdt, drifting):
    """`-t each`'s pool path on the drifting platform of tests/test_gpu_windows.py: pdt_demod_windows_held, then pdt_tones_batch with
    count = 1.  14 records whose frequencies fall monotonically and meet the bound of tests/test_tones.py against the synthesiser's
    closed form; the payloads decode as they do without the measurement."""
    x, p = drifting
    sent = {bytes(pdt.synth_argos_payload(p, b)) for b in range(2, 16)}
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x), IN_RATE, len(x))
        assert len(windows) == 14
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, 0.0) for _ in windows]
        try:
            holder.demod_windows_held(ds, windows)
            before = [d.frames_array().tobytes() for d in ds]
            tones = pdt.tones_batch(ds, count=1, cap=1)
            each = {bytes(f["bytes"][:7]) for d in ds for f in d.frames_array() if f["complete"]}
            assert [d.frames_array().tobytes() for d in ds] == before
            for d, w, t in zip(ds, windows, tones):                      # the kernel on the window's stream is the hook on it
                assert t.tobytes() == pdt.host_tones(FS, w.offset_hz, d.stage(pdt.ST_CHANNEL, 0, 4096), search_hz=ARGOS_RANGE, count=1).tobytes()
        finally:
            for d in ds:
                d.close()
    assert [len(t) for t in tones] == [1] * 14
    rec = np.concatenate(tones)
    err = np.array([t["freq_hz"] - truth_hz(p, IN_RATE, w.first_frame + t["time_s"] * IN_RATE) for t, w in zip(rec, windows)])
    print("freq_hz - 250 kHz:", (rec["freq_hz"] - 250000.0).round(2), "worst |error|", np.abs(err).max().round(4), "Hz, C/N0", rec["cn0_dbhz"].round(1),
          "decoded:", len(each & sent))
    assert np.all(rec["valid"] == 1) and np.all(np.diff(rec["freq_hz"]) < 0)
    assert np.abs(err).max() <= ARGOS_FREQ_BOUND_HZ
    assert len(each & sent) >= 12 and each <= sent                       # (tests/test_gpu_windows.py's figure)


def test_command_line_measure(pdt, drifting, tmp_path):
    x, p = drifting
    wav = str(tmp_path / "drift.wav")
    pdt.write_wav(wav, IN_RATE, x)
    exe = os.path.join(BIN, "demodARGOS")
    out, out_m, m = str(tmp_path / "out"), str(tmp_path / "out_m"), str(tmp_path / "m.txt")
    r0 = subprocess.run([exe, "-x", str(D), "-t", "each", "-o", out, wav], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run([exe, "-x", str(D), "-t", "each", "-M", m, "-o", out_m, wav], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r1.returncode == 0, r1.stdout[-2000:]
    assert open(out, "rb").read() == open(out_m, "rb").read() and os.path.getsize(out) > 300
    assert r0.stdout == r1.stdout                                        # the burst lines are the same
    lines = [l.split() for l in open(m).read().splitlines()]
    assert len(lines) == 14 and all(len(l) == 5 for l in lines)
    idx, t, f, cn0, lvl = (np.array([float(l[k]) for l in lines]) for k in range(5))
    assert list(idx) == list(range(14)) and np.all(np.diff(t) > 1.4) and np.all(np.diff(f) < 0)
    assert np.all(np.abs(f - np.array([truth_hz(p, IN_RATE, ts * IN_RATE) for ts in t])) <= ARGOS_FREQ_BOUND_HZ + 0.005 + 0.6 * 114.3e-5)   # (%.2f; %.5f s of a 114.3 Hz/s ramp)
    assert np.all(cn0 > 70.0) and np.all(lvl < 0.0)
    # a pool of 4: four rounds, the same lines
    m4 = str(tmp_path / "m4.txt")
    r4 = subprocess.run([exe, "-x", str(D), "-t", "each:4", "-M", m4, "-o", out_m, wav], capture_output=True, text=True, timeout=300)
    assert r4.returncode == 0 and open(m4).read() == open(m).read()
    # one channel along the capture: a line per segment at stride N, without the index
    mc = str(tmp_path / "mc.txt")
    rc = subprocess.run([exe, "-x", str(D), "-t", "250", "-P", "-M", mc, "-o", out_m, wav], capture_output=True, text=True, timeout=300)
    assert rc.returncode == 0, rc.stdout[-2000:]
    seg = [l.split() for l in open(mc).read().splitlines()]
    assert len(seg) == len(x) // D // 4096 and all(len(l) == 4 for l in seg) and float(seg[1][0]) - float(seg[0][0]) == pytest.approx(0.128)
    # not from a pipe, not with -l, not without -x: the message, exit status 1, no file
    for args in (["-l", "-x", str(D), "-t", "250", "-M", mc + "x", "-"], ["-l", "-x", str(D), "-t", "250", "-M", mc + "x", wav], ["-M", mc + "x", wav]):
        rb = subprocess.run([exe, "-o", out_m + "x"] + args, capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
        assert rb.returncode == 1 and "-M needs a wideband capture file" in rb.stdout and not os.path.exists(mc + "x")
