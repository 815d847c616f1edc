"""The carrier survey on the GPU: the kernels' averaged spectrum against the host restatement bit for bit, survey -> set_channel ->
demod_channels on the captures of the channel tests, that a survey leaves no trace in a context, and `-t auto` on the command line
(DESIGN 4.12)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_channel_input import SETUPS, carriers, fmt_code, random_capture, to_cu8
from test_gpu_real_input import transmitted

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
FORMATS = ("pcm16", "f32", "cu8", "cs8")
RUN = 64                                                                # SURVEY_RUN of csrc/pdt_survey.h


def noisy_tone(rng, fmt: str, n: int) -> np.ndarray:
    """A carrier of amplitude 0.2 at 0.2345 of the rate in uniform noise of +-0.3 (so that the carriers compare too), in format fmt."""
    z = 0.2 * np.exp(2j * np.pi * 0.2345 * np.arange(n)) + 0.3 * (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n))
    f = np.stack([z.real, z.imag], axis=1)
    if fmt == "f32":
        return f.astype(np.float32)
    if fmt == "pcm16":
        return np.round(f * 32767.0).astype(np.int16)
    if fmt == "cu8":
        return np.clip(np.round(f * 128.0 + 127.5), 0, 255).astype(np.uint8)
    return np.clip(np.round(f * 128.0), -128, 127).astype(np.int8)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("nfft", (1024, 4096, 16384))
def test_kernels_equal_host_restatement(pdt, nfft, fmt):
    """pdt_survey_spectrum after pdt_survey / pdt_survey_device is pdt_host_survey's spectrum, bit for bit, and the carriers are equal:
    one segment, one run of R segments, R + 1 segments and a long capture with a partial segment behind it; a stretch of a capture;
    resident captures 1, 2 and 3 samples behind a 16-byte boundary."""
    rng = np.random.default_rng(nfft + FORMATS.index(fmt))
    in_rate, fs, D = 1000000, 250000, 4
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.set_channel(D, 0.0)
        # full-scale random samples: the widest range of values through the transform
        x = random_capture(rng, fmt, 2 * nfft + 1)
        want, found = pdt.host_survey(in_rate, 4500.0, fs, x, nfft=nfft)
        assert d.survey(x, nfft=nfft) == found
        assert d.survey_spectrum().tobytes() == want.tobytes()
        for nseg, extra in ((1, 0), (RUN, 0), (RUN + 1, 3), (3 * RUN + 5, 77)):
            x = noisy_tone(rng, fmt, nseg * nfft + extra)
            want, found = pdt.host_survey(in_rate, 4500.0, fs, x, nfft=nfft)
            got = d.survey(x, nfft=nfft)
            assert d.survey_spectrum().tobytes() == want.tobytes(), (nseg, extra)
            assert got == found and len(found) >= 1
        # a stretch of the last (long) capture
        want, found = pdt.host_survey(in_rate, 4500.0, fs, x, nfft=nfft, first_frame=1001, nframes=(RUN + 3) * nfft + 5)
        assert d.survey(x, nfft=nfft, first_frame=1001, nframes=(RUN + 3) * nfft + 5) == found
        assert d.survey_spectrum().tobytes() == want.tobytes()
        # resident captures whose first sample sits 1, 2 and 3 samples behind a 16-byte boundary
        n = (RUN + 2) * nfft + 9
        dev = torch.from_numpy(x[: n + 3].reshape(-1).copy()).to("cuda:0")
        torch.cuda.synchronize()
        for skip in (0, 1, 2, 3):
            want, found = pdt.host_survey(in_rate, 4500.0, fs, x[skip: skip + n], nfft=nfft)
            got = d.survey_device(dev.data_ptr() + skip * 2 * x.itemsize, n, fmt_code(pdt, x), nfft=nfft)
            assert d.survey_spectrum().tobytes() == want.tobytes(), skip
            assert got == found
        # surveyed and never demodulated: no frames, no channel stage
        assert len(d.frames_array()) == 0 and d.stage_len(pdt.ST_CHANNEL) == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_capture_aligned_to_its_element_but_not_to_its_pair(pdt, fmt):
    """A resident capture that begins half a sample off a pair boundary (a multiple of the element's size: 2 bytes for int16, 4 for
    float, 1 for the 8-bit formats): k_spectra loads every segment sample by sample (head = N), and the spectrum is pdt_host_survey's
    of the same bytes.  More than one run of segments, 0, 1 and 3 whole samples further on too."""
    rng = np.random.default_rng(500 + FORMATS.index(fmt))
    in_rate, fs, D, nfft = 1000000, 250000, 4, 1024
    n = (RUN + 1) * nfft + 9
    flat = noisy_tone(rng, fmt, n + 4).reshape(-1)                         # elements: I, Q, I, Q, ...
    dev = torch.from_numpy(flat.view(np.uint8).copy()).to("cuda:0")        # (the bytes; torch allocations are 16-byte aligned)
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.set_channel(D, 0.0)
        for skip in (0, 1, 3):
            first = 2 * skip + 1                                           # the capture begins with what was a Q
            host = flat[first: first + 2 * n].reshape(n, 2)
            want, found = pdt.host_survey(in_rate, 4500.0, fs, host, nfft=nfft)
            got = d.survey_device(dev.data_ptr() + first * flat.itemsize, n, fmt_code(pdt, flat), nfft=nfft)
            assert d.survey_spectrum().tobytes() == want.tobytes(), skip
            assert got == found


def test_changing_nfft_on_one_context(pdt):
    """The window and the twiddles are kept on the context under one key, nfft: 1024, then 16384, then 1024 again on ONE context,
    each spectrum pdt_host_survey's."""
    rng = np.random.default_rng(99)
    in_rate, fs, D = 1000000, 250000, 4
    x = noisy_tone(rng, "pcm16", (RUN + 1) * 16384 + 5)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.set_channel(D, 0.0)
        for nfft in (1024, 16384, 1024):
            want, found = pdt.host_survey(in_rate, 4500.0, fs, x, nfft=nfft)
            got = d.survey(x, nfft=nfft)
            assert d.survey_spectrum().tobytes() == want.tobytes(), nfft
            assert got == found and len(found) >= 1


def test_arguments(pdt):
    fs = 250000
    x = np.zeros((2 * 16384, 2), dtype=np.int16)
    L = pdt.lib()
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.survey(x)                                                 # no channel yet
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.survey_spectrum()                                         # no survey yet
        d.set_channel(4, 123456.0)
        assert d.survey(x) == []
        assert d.survey_spectrum().shape == (16384,)
        assert L.pdt_survey_spectrum(d._h, np.zeros(4096, dtype=np.float32).ctypes.data, 4096) == -1
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.survey(x, nfft=2048)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.survey(x[:16383])
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.survey(x, first_frame=16385)
        rec, count = (pdt.CarrierRec * 4)(), pdt.C.c_int(0)
        for fmt in (0, 1, 2, 3, 15, 20):
            assert L.pdt_survey(d._h, x.ctypes.data, len(x), fmt, None, rec, 4, pdt.C.byref(count)) == -1
        assert L.pdt_survey(d._h, x.ctypes.data, len(x), 16, None, rec, 0, pdt.C.byref(count)) == -1


@pytest.mark.parametrize("rendering", ["pcm16", "cu8"])
@pytest.mark.parametrize("in_rate,D,offsets", SETUPS)
def test_survey_then_demodulate(pdt, in_rate, D, offsets, rendering):
    """The SETUPS captures at 8 s, resident: survey, set_channel to the found offsets, demod_channels.  Every channel's complete frames
    are frames the generator sent and its PLL locks within its range; and each context holds, byte for byte, what a context given
    the same offsets as numbers holds without any survey."""
    fs = in_rate // D
    x, params = carriers(pdt, 0, in_rate, 8.0, offsets, (11, 12), 1000.0)
    if rendering == "cu8":
        x = to_cu8(x)
    dev = torch.from_numpy(x.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    fmt = fmt_code(pdt, x)
    ds = [pdt.Demodulator(pdt.MODE_POES, fs).set_channel(D, 0.0) for _ in offsets]
    plain = []
    try:
        found = ds[0].survey_device(dev.data_ptr(), len(x), fmt)
        assert len(found) == 2
        for d, c in zip(ds, found):
            d.set_channel(D, c.offset_hz)
        pdt.demod_channels(ds, dev.data_ptr(), len(x), fmt)
        for d, c in zip(ds, found):
            near = int(np.argmin([abs(c.offset_hz - (off + 1000.0)) for off in offsets]))
            assert abs(c.offset_hz - (offsets[near] + 1000.0)) <= in_rate / 16384
            res = transmitted(pdt, params[near], d.frames_array(), len(x), in_rate)
            st = d.stats()
            print(in_rate, D, rendering, c, res, st.lock_freq_hz)
            assert res["ok"], res
            assert st.lock_sample >= 0 and abs(st.lock_freq_hz) < 4500.0
        plain = [pdt.Demodulator(pdt.MODE_POES, fs).set_channel(D, c.offset_hz) for c in found]
        pdt.demod_channels(plain, dev.data_ptr(), len(x), fmt)
        for d, e in zip(ds, plain):
            assert d.text() == e.text() and len(d.text()) > 10000
            assert d.frames_array().tobytes() == e.frames_array().tobytes()
            assert d.stage(pdt.ST_CHANNEL).tobytes() == e.stage(pdt.ST_CHANNEL).tobytes()
    finally:
        for d in ds + plain:
            d.close()


def test_command_line_auto(pdt, tmp_path):
    in_rate = 1000000
    x, _ = carriers(pdt, 0, in_rate, 6.0, (200000.0, -180000.0), (11, 12), 1000.0)
    wav = str(tmp_path / "capture.wav")
    pdt.write_wav(wav, in_rate, x)
    exe = os.path.join(BIN, "demodPOES")
    out = str(tmp_path / "auto.txt")
    r = subprocess.run([exe, "-x", "4", "-t", "auto", "-o", out, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = re.findall(r"^Channel (\d+) at ([+-][0-9.]+) Khz \(found, ([0-9.]+) dB over the floor\)$", r.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == [0, 1]
    khz = [l[1] for l in lines]
    assert sorted(round(float(k)) for k in khz) == [-179, 201]
    num = str(tmp_path / "numbers.txt")
    r = subprocess.run([exe, "-x", "4", "-t", khz[0], "-t", khz[1], "-o", num, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    for i in (0, 1):
        a, b = open(f"{out}.{i}", "rb").read(), open(f"{num}.{i}", "rb").read()
        assert a == b and len(a) > 10000
    # the strongest carrier alone: the usual single output file
    one = str(tmp_path / "one.txt")
    r = subprocess.run([exe, "-x", "4", "-t", "auto:1", "-o", one, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(one, "rb").read() == open(f"{out}.0", "rb").read()
    # noise: one line, no file, exit status 1
    p = pdt.synth_params(0, in_rate, 1000.0, 5)
    p.amplitude = 0
    noise = np.zeros((2000000, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(pdt.C.byref(p), 0, len(noise), noise.ctypes.data)
    nwav = str(tmp_path / "noise.wav")
    pdt.write_wav(nwav, in_rate, noise)
    nout = str(tmp_path / "noise.txt")
    r = subprocess.run([exe, "-x", "4", "-t", "auto", "-o", nout, nwav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1
    assert re.search(r"^No carrier found \(strongest bin [0-9.]+ dB over the floor\)$", r.stdout, flags=re.M)
    assert not os.path.exists(nout) and not any(f.startswith("noise.txt") for f in os.listdir(tmp_path))
    # auto beside a number, auto without -x, auto from a pipe
    r = subprocess.run([exe, "-x", "4", "-t", "auto", "-t", "200", "-o", nout, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot be combined" in r.stdout and not os.path.exists(nout)
    r = subprocess.run([exe, "-x", "4", "-t", "200", "-t", "auto", "-o", nout, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "cannot be combined" in r.stdout and not os.path.exists(nout)
    r = subprocess.run([exe, "-t", "auto", "-o", nout, wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "-t requires -x" in r.stdout
    r = subprocess.run([exe, "-l", "-x", "4", "-t", "auto", "-s", "1000", "-o", nout, "-"], input="", capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "needs a capture file" in r.stdout and not os.path.exists(nout)
