"""Feed-forward ARGOS bits on the GPU: k_ff_mix, k_ff_search and k_ff_pick against the host restatement, byte for byte --
sync record, characters, soft bit patterns, sample indices -- on every stream of the CPU tests, the real recording both ways round, bursts
at a wrong bit rate, other sample rates, a stream longer than two seconds; three contexts in one batch against three single calls; the
per-burst windows of a wideband capture, every message right and everything else the contexts hold left as it was; -b on the command
line; error codes."""
import os
import subprocess

import numpy as np
import pytest

import argos_best_cases as bc
import ff_cases as fc
import real_captures as rc
from conftest import ROOT
from test_gpu_bursts import STAT_FIELDS
from test_windows import D, FS, IN_RATE, to_cu8

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
PAIR, SECONDS = (202, 206), 6.0


@pytest.fixture(scope="module")
def argos(pdt):
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as d:
        yield d


def held(pdt, d):
    """what a context holds after a whole-capture call: frames, text, the statistics of the capture (not the process-wide allocation
    time) and the length and bytes of every stage"""
    st = d.stats()
    stages = tuple((d.stage_len(s), d.stage(s).tobytes() if d.stage_len(s) else b"") for s in range(pdt.ST_CHANNEL + 1))
    return d.frames_array().tobytes(), d.text(), tuple(getattr(st, f) for f in STAT_FIELDS), stages


def stage_equals_host(pdt, d, fs, y, **cfg):
    got, want = d.stage_ff_bits(fs, y, **cfg), pdt.host_ff_bits(fs, y, **cfg)
    assert fc.same_bits(got, want), (fs, len(y), cfg, got.sync, want.sync)
    assert fc.same_bits(d.ff_read(), want)
    return got


@pytest.mark.parametrize("H", (4, 10, 40))
def test_stage_equals_host_on_small_streams(pdt, argos, H):
    fs = 800 * H
    for name, y in fc.small_streams(H):
        for R in (0, 2):
            stage_equals_host(pdt, argos, fs, y, rate_steps=R, residual_hz=0.0)
        stage_equals_host(pdt, argos, fs, y, rate_steps=2, rate_step_ppm=20000.0, residual_hz=-123.456)
        got = stage_equals_host(pdt, argos, fs, y, rate_steps=1)                       # measured: too short for a tone's segment
        assert (got.sync["tone_valid"], got.sync["residual_hz"]) == (0, 0.0), name


@pytest.mark.parametrize("mirrored", (False, True))
def test_stage_on_the_real_recording(pdt, argos, mirrored):
    y = fc.real(mirrored)
    for R in (20, 0):
        got = stage_equals_host(pdt, argos, 32000, y, rate_steps=R)
        assert got.sync["tone_valid"] == 1
        for rule in (0, 1):
            assert fc.decoded(pdt, got.bits, rule) == [fc.REAL_MESSAGE + (0 if mirrored else 1,)]
    assert fc.same_bits(stage_equals_host(pdt, argos, 32000, y), pdt.host_ff_bits(32000, y, rate_steps=20))      # the defaults


def test_stage_on_bursts_at_a_wrong_bit_rate(pdt, argos):
    for e in fc.RATE_ERRORS:
        assert fc.burst_decodes(pdt, stage_equals_host(pdt, argos, fc.BURST_FS, fc.burst(e)).bits), e
    assert fc.burst_decodes(pdt, stage_equals_host(pdt, argos, fc.BURST_FS, fc.burst(0.0), rate_steps=0).bits)
    assert not fc.burst_decodes(pdt, stage_equals_host(pdt, argos, fc.BURST_FS, fc.burst(0.004), rate_steps=0).bits)


@pytest.mark.parametrize("fs,e,steps", ((8000, 0.004, (20, 0)), (48000, 0.004, (20, 0)), (102400, 0.001, (3,))))
def test_stage_at_other_rates(pdt, argos, fs, e, steps):
    """H = 10, 60 (two wavefronts, the second partly filled) and 128 (four full ones, the largest tile)"""
    y = fc.burst(e, fs=fs)
    for R in steps:
        got = stage_equals_host(pdt, argos, fs, y, rate_steps=R)
        assert fc.burst_decodes(pdt, got.bits) == (R != 0)


def test_stage_on_a_stream_longer_than_two_seconds(pdt, argos):
    fs = 8000
    rng = np.random.default_rng(12)
    y = np.concatenate([fc.burst(0.0, fs=fs), 0.05 * rng.standard_normal((2 * fs, 2)).astype(np.float32)])
    assert len(y) > 2 * fs + 1000
    got = stage_equals_host(pdt, argos, fs, y)
    assert fc.same_bits(got, pdt.host_ff_bits(fs, y[: 2 * fs])) and got.index[-1] <= 2 * fs and len(got.bits) >= 780
    assert fc.burst_decodes(pdt, got.bits)


@pytest.fixture(scope="module")
def pair(pdt):
    return bc.kind2_pair(pdt, PAIR, SECONDS)


@pytest.fixture(scope="module")
def windows(pdt, pair):
    """the capture's bursts, each demodulated in a window and a context of its own (the first one profiled): (windows, contexts)"""
    x, _ = pair
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        win = pdt.burst_windows(holder.bursts(x), IN_RATE, len(x))
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS, profile=(i == 0)).set_channel(D, 0.0) for i in range(len(win))]
        try:
            holder.demod_windows_held(ds, win)
            yield win, ds
        finally:
            for d in ds:
                d.close()


def test_batch_of_three_equals_three_single_calls(pdt, windows):
    _, ds = windows
    three = ds[:3]
    syncs = pdt.ff_bits_batch(three)
    times = ds[0].kernel_times()
    assert [times[k][0] for k in ("k_ff_mix", "k_ff_search", "k_ff_pick")] == [1, 1, 1]
    batch = [d.ff_read() for d in three]
    for d, s, b in zip(three, syncs, batch):
        assert d.ff_bits().tobytes() == s.tobytes() == b.sync.tobytes()
        assert fc.same_bits(d.ff_read(), b) and len(b.bits) > 100
    times = ds[0].kernel_times()
    assert [times[k][0] for k in ("k_ff_mix", "k_ff_search", "k_ff_pick")] == [1, 1, 1]
    assert len({b.sync.tobytes() for b in batch}) == 3


def test_wideband_windows(pdt, pair, windows):
    """seeds (202, 206), 6 s: the chain loses the window at frame 4 620 288 under either rule; feed-forward bits give every window's
    message, equal to the host restatement on each context's own channel stream, and leave everything else the contexts hold alone"""
    x, params = pair
    win, ds = windows
    assert len(win) == 8 and 4620288 in [w.first_frame for w in win]
    before = [held(pdt, d) for d in ds]
    tones = [t.tobytes() for t in pdt.tones_batch(ds, cap=1)]
    loop = [m.tobytes() for m in pdt.argos_messages_batch(ds)]
    msgs, syncs = pdt.ff_messages_batch(ds, with_sync=True)
    for d, m, s in zip(ds, msgs, syncs):
        tone = d.tones(cap=1)
        assert len(tone) == 1 and tone[0]["valid"]
        want = pdt.host_ff_bits(FS, d.stage(pdt.ST_CHANNEL), residual_hz=float(tone[0]["residual_hz"]))
        assert s.tobytes() == want.sync.tobytes() and fc.same_bits(d.ff_read(), want)
        host = pdt.host_argos_messages(want.bits.tobytes())
        host["time_src"] = want.index[host["bit_index"]]
        host["time"] = host["time_src"] / FS
        assert m.tobytes() == host.tobytes()
    right, wrong, lost = bc.tally(pdt, params, win, msgs)
    print("feed-forward, rule 0: windows right", right, "of", len(win), "wrong", wrong)
    assert (right, wrong, lost) == (8, 0, [])
    right1, wrong1, _ = bc.tally(pdt, params, win, pdt.ff_messages_batch(ds, rule=pdt.ARGOS_RULE_BEST))
    assert (right1, wrong1) == (8, 0)
    assert [m.tobytes() for m in msgs] == [d.ff_messages().tobytes() for d in ds]
    assert [held(pdt, d) for d in ds] == before
    assert [t.tobytes() for t in pdt.tones_batch(ds, cap=1)] == tones
    assert [m.tobytes() for m in pdt.argos_messages_batch(ds)] == loop
    loop_right, _, _ = bc.tally(pdt, params, win, pdt.argos_messages_batch(ds))
    print("the loop's bits, rule 0: windows right", loop_right, "of", len(win))
    assert loop_right < 8


def test_command_line(pdt, pair, windows, tmp_path):
    exe = os.path.join(BIN, "demodARGOS")
    x, params = pair
    win, ds = windows
    # the real recording, uncut: its line
    out = str(tmp_path / "real.txt")
    r = subprocess.run([exe, "-A", out, "-b", "-o", str(tmp_path / "real.packets"), rc.PACKET_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    want = pdt.host_ff_bits(32000, fc.real(False))
    at = int(want.index[97])
    assert open(out, "rb").read() == b"%.5fi 1 01D81 00 55 AA FF\n" % (at / 32000.0)
    # the window capture: its 8 lines, times from the capture's start
    x8 = to_cu8(x)
    cu8 = str(tmp_path / "capture.cu8")
    x8.tofile(cu8)
    out = str(tmp_path / "each.txt")
    r = subprocess.run([exe, "-x", str(D), "-s", str(IN_RATE // 1000), "-t", "each", "-A", out, "-b", "-o", str(tmp_path / "each.packets"), cu8],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        win8 = pdt.burst_windows(holder.bursts(x8, max_s=5.0), IN_RATE, len(x8))
        cs = [pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, 0.0) for _ in win8]
        try:
            holder.demod_windows_held(cs, win8)
            parts = pdt.ff_messages_batch(cs, cap=16)
            for part, w in zip(parts, win8):
                part["time"] += w.first_frame / IN_RATE
        finally:
            for c in cs:
                c.close()
    text = open(out, "rb").read()
    assert text == pdt.format_argos_messages(np.concatenate(parts)) and text.count(b"\n") == 8
    assert bc.tally(pdt, params, win8, parts)[:2] == (8, 0)
    # where -b is refused
    for args in (["-b", rc.PACKET_WAV], ["-A", out + "x", "-b", "-l", rc.PACKET_WAV], ["-A", out + "x", "-b", "-x", "32", "-s", "1024", "-t", "bursts", cu8]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "-b needs demodARGOS" in r.stdout and not os.path.exists(out + "x"), args
    r = subprocess.run([os.path.join(BIN, "demodPOES"), "-A", out + "x", "-b", rc.PACKET_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "-b needs demodARGOS" in r.stdout and not os.path.exists(out + "x")


def test_errors_and_states(pdt, argos, windows):
    _, ds = windows
    y = fc.burst(0.0)
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as fresh:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            fresh.ff_read()
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            fresh.ff_bits()                                                           # no channel stream yet
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            fresh.ff_messages()
        for fs in (0, 800, 44100, 800 * 129):
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                fresh.stage_ff_bits(fs, y)
        for cfg in (dict(rate_steps=33), dict(rate_steps=-1), dict(rate_step_ppm=-1.0), dict(residual_hz=float("nan")), dict(residual_hz=8000.0),
                    dict(rate_steps=32, rate_step_ppm=4000.0)):
            with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
                fresh.stage_ff_bits(fc.BURST_FS, y, **cfg)
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            fresh.ff_read()                                                           # a refused call leaves no bits
        fresh.stage_ff_bits(fc.BURST_FS, y)
        assert len(fresh.ff_read().bits) > 300
    with pdt.Demodulator(pdt.MODE_POES, 32000) as poes:
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.stage_ff_bits(fc.BURST_FS, y)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.ff_bits()
    before = held(pdt, ds[0])
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        pdt.ff_bits_batch([ds[0], ds[1], ds[0]])                                      # not distinct
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        pdt.ff_messages_batch([ds[0]], rule=2)
    with pdt.Demodulator(pdt.MODE_ARGOS, 16000) as other:
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.ff_bits_batch([ds[0], other])                                         # another sample rate
    with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
        pdt.ff_bits_batch([ds[0], argos])                                             # one of them without a channel stream
    assert pdt.ff_bits_batch([]).shape == (0,) and pdt.ff_messages_batch([]) == []
    assert held(pdt, ds[0]) == before
