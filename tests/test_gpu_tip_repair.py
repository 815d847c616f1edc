"""The repair of failed TIP parity groups on the GPU: k_tip_repair against the host restatement byte for byte -- records,
info, summary -- on every hand-built case of tests/tip_repair_cases.py and on the 300 random records; pdt_tip_repair behind
pdt_stage_ffp_frames against the host chain on a weak synthetic capture whose frames carry parity and on the real recording; states and
arguments; a context's other results untouched; the command line's -Q on both -b routes."""
import os
import subprocess

import numpy as np
import pytest

import tip_repair_cases as rc
from conftest import ROOT
from test_gpu_bursts import STAT_FIELDS

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
CLIP_WAV = os.path.join(ROOT, "tests", "golden", "5sec_clip.wav")


@pytest.fixture(scope="module")
def poes(pdt):
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        yield d


@pytest.fixture(scope="module")
def hand(pdt):
    return rc.hand_cases(pdt)


@pytest.fixture(scope="module")
def weak(pdt):
    """kind 3, 50 ksps, 3 s, seed 1234, noise x 9: the capture, its float stream, and the host chain's bits, frames and repair"""
    p, x = rc.weak_capture(pdt, 3, 9.0, seconds=3.0)
    got, fr = rc.ffp_frames_host(pdt, 50000, x)
    return x, x.astype(np.float32) / np.float32(32768.0), got, fr, pdt.host_tip_repair(got.soft, fr)


@pytest.mark.parametrize("k", range(18))
def test_stage_equals_host_on_the_hand_built_cases(pdt, poes, hand, k):
    c = hand[k]
    assert rc.same(poes.stage_tip_repair(c["soft"], c["frames"]), pdt.host_tip_repair(c["soft"], c["frames"])), c["name"]


def test_stage_equals_host_on_random_records(pdt, poes):
    c = rc.random_case(pdt)
    got = poes.stage_tip_repair(c["soft"], c["frames"])
    assert rc.same(got, pdt.host_tip_repair(c["soft"], c["frames"])) and got[2]["repaired"] > 500


def test_after_the_feed_forward_frames_on_the_weak_capture(pdt, poes, weak):
    x, y, got, fr, want = weak
    mine = poes.stage_ffp_frames(50000, y)
    assert mine["bytes"].tobytes() == fr["bytes"].tobytes() and len(fr) > 20
    out = poes.tip_repair(mine)
    assert want[2]["failing"] > 3 and out[2] == want[2] and out[1].tobytes() == want[1].tobytes()
    assert out[0]["bytes"].tobytes() == want[0]["bytes"].tobytes() and out[0]["bit_index"].tolist() == want[0]["bit_index"].tolist()
    for name in ("time", "time_src", "inverted", "nbytes", "complete"):
        assert out[0][name].tobytes() == mine[name].tobytes()
    # the stage entry on the same soft values: the same bytes, and the feed-forward bits of the context stay
    assert rc.same(poes.stage_tip_repair(got.soft, fr), want)
    assert poes.ffp_read().soft.tobytes() == got.soft.tobytes()


def test_after_the_feed_forward_frames_on_the_real_recording(pdt, poes, clip):
    rate, iq = clip
    got, fr = rc.ffp_frames_host(pdt, rate, iq)
    mine = poes.stage_ffp_frames(rate, iq.astype(np.float32) / np.float32(32768.0))
    out, want = poes.tip_repair(mine), pdt.host_tip_repair(got.soft, fr)
    assert len(mine) == 49 and out[2] == want[2] and out[1].tobytes() == want[1].tobytes() and out[0]["bytes"].tobytes() == want[0]["bytes"].tobytes()
    assert out[2] == dict(checked=49, skipped=0, failing=0, repaired=0)


def test_errors_and_states(pdt, hand, clip):
    c = hand[0]
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_repair(c["frames"])                                         # no feed-forward call yet
        assert rc.same(d.stage_tip_repair(c["soft"], c["frames"]), pdt.host_tip_repair(c["soft"], c["frames"]))   # ... the stage entry needs none
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_repair(c["frames"])                                         # ... and leaves no bits behind
        L, sm = pdt.lib(), pdt.TipRepairSummary()
        fr, soft = c["frames"].copy(), c["soft"].copy()
        assert L.pdt_tip_repair(d._h, None, 1, None, sm) == -1 and L.pdt_tip_repair(d._h, fr.ctypes.data, 1, None, None) == -1
        assert L.pdt_tip_repair(d._h, fr.ctypes.data, 1 << 31, None, sm) == -1
        assert L.pdt_stage_tip_repair(d._h, None, 5, fr.ctypes.data, 1, None, sm) == -1
        assert L.pdt_stage_tip_repair(d._h, soft.ctypes.data, soft.size, None, 1, None, sm) == -1
        assert L.pdt_stage_tip_repair(d._h, soft.ctypes.data, soft.size, fr.ctypes.data, 1, None, None) == -1
        assert L.pdt_stage_tip_repair(d._h, soft.ctypes.data, 1 << 31, fr.ctypes.data, 1, None, sm) == -1
        assert L.pdt_stage_tip_repair(d._h, soft.ctypes.data, soft.size, fr.ctypes.data, 1 << 31, None, sm) == -1
        assert L.pdt_stage_tip_repair(d._h, soft.ctypes.data, soft.size, fr.ctypes.data, 1, None, sm) == 0 and sm.repaired == 1   # (info is optional)
        d.stage_ffp_bits(50000, clip[1][:20000].astype(np.float32) / np.float32(32768.0))
        d.tip_repair(c["frames"])                                             # now there are bits
        d.stream_begin()
        d.stream_push(clip[1][:20000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_repair(c["frames"])                                         # an open stream
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.stage_tip_repair(c["soft"], c["frames"])
        d.stream_end()
    with pdt.Demodulator(pdt.MODE_ARGOS, 51200) as argos:
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.tip_repair(c["frames"])                                     # an ARGOS context
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.stage_tip_repair(c["soft"], c["frames"])


def test_nothing_else_of_the_context_changes(pdt, clip, weak):
    x = np.repeat(weak[0], 2, axis=0)                                         # (the capture at twice its rate: a zero-order hold)
    with pdt.Demodulator(pdt.MODE_POES, 50000, profile=True) as d:
        d.set_channel(2, 0.0).demod_channel(x)
        fr = d.ffp_frames()
        assert "k_tip_repair" not in d.kernel_times()

        def state():
            s, b = d.stats(), d.ffp_read()
            return (d.text(), d.frames_array().tobytes(), d.stage(pdt.ST_BITS).tobytes(), tuple(getattr(s, f) for f in STAT_FIELDS), b.sync.tobytes(),
                    b.bits.tobytes(), b.soft.tobytes(), b.index.tobytes(), b.blocks.tobytes(), d.tip_sync().tobytes())

        before = state()
        out, info, sm = d.tip_repair(fr)
        assert state() == before
        assert rc.same((out, info, sm), pdt.host_tip_repair(d.ffp_read().soft, fr)) and sm["checked"] == len(fr) > 20 and sm["failing"] > 0
        times = d.kernel_times()
        assert times["k_tip_repair"][0] == 1 and times["k_tip_repair"][1] >= 0
        d.stage_tip_repair(weak[2].soft, weak[3])
        assert state() == before


def report_lines(fr, info):
    lines = []
    for r, i in zip(fr, info):
        if i["failed"]:
            lines.append(f"{float(r['time']):.5f}" + "".join(f" {g} {int(i['pos'][g])} {float(i['least'][g]):.9g} {float(i['next'][g]):.9g}"
                                                           for g in range(5) if int(i["failed"]) >> g & 1))
    return lines


def write_wav(path, rate, x):
    hdr = bytearray(open(CLIP_WAV, "rb").read(44))
    hdr[4:8] = (x.nbytes + 36).to_bytes(4, "little")
    hdr[24:28] = int(rate).to_bytes(4, "little")
    hdr[28:32] = (int(rate) * 4).to_bytes(4, "little")
    hdr[40:44] = (x.nbytes).to_bytes(4, "little")
    open(path, "wb").write(bytes(hdr) + x.astype("<i2").tobytes())


def test_command_line(pdt, poes, clip, weak, tmp_path):
    exe = os.path.join(BIN, "demodPOES")
    out, fly, rep = str(tmp_path / "minor.txt"), str(tmp_path / "fly.txt"), str(tmp_path / "repair.txt")
    # the real recording, a plain I,Q file: 49 frames, none with a failing group
    r = subprocess.run([exe, "-q", "-b", "-W", fly, "-Q", rep, "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    want = poes.stage_ffp_frames(50000, clip[1].astype(np.float32) / np.float32(32768.0))
    assert len(want) == 49 and open(fly, "rb").read() == pdt.format_frames(want) and open(rep).read() == ""
    assert f"Parity repair: 49 records checked, 0 skipped, 0 with a failing group, 0 groups repaired -> {rep}" in r.stdout
    assert r.stdout.index("Parity repair: ") < r.stdout.index("Flywheel frames: 49 -> ")
    assert "Flywheel: 49 out of 49 Error Free Frames" in r.stdout and "passes by construction" in r.stdout
    # the weak capture whose frames carry parity, a plain file: the repaired frames and a report with lines
    x, y = weak[0], weak[1]
    plain = str(tmp_path / "weak.wav")
    write_wav(plain, 50000, x)
    r = subprocess.run([exe, "-b", "-W", fly, "-Q", rep, "-o", out, plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    mine = poes.stage_ffp_frames(50000, y)
    fixed, info, sm = poes.tip_repair(mine)
    assert sm["failing"] > 3 and open(fly, "rb").read() == pdt.format_frames(fixed) != pdt.format_frames(mine)
    got = open(rep).read().split("\n")
    assert got[-1] == "" and got[:-1] == report_lines(mine, info) and len(got) - 1 == sm["failing"]
    for line in got[:-1]:                                                     # the format of INTEGRATION 2.16: a time, then four fields per failing group
        f = line.split()
        assert len(f) % 4 == 1 and float(f[0]) >= 0
        for k in range(1, len(f), 4):
            assert 0 <= int(f[k]) <= 4 and int(f[k + 1]) in rc.candidates(int(f[k])) and 0 <= float(f[k + 2]) <= float(f[k + 3])
    assert (f"Parity repair: {sm['checked']} records checked, {sm['skipped']} skipped, {sm['failing']} with a failing group, {sm['repaired']} groups "
            f"repaired -> {rep}") in r.stdout
    # the channel stream of a wideband capture
    wide = str(tmp_path / "wide.wav")
    xx = np.repeat(x, 2, axis=0)
    write_wav(wide, 100000, xx)
    r = subprocess.run([exe, "-x", "2", "-t", "0", "-b", "-W", fly, "-Q", rep, "-o", out, wide], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        d.set_channel(2, 0.0).demod_channel(xx)
        mine = d.ffp_frames()
        fixed, info, sm = d.tip_repair(mine)
    assert sm["failing"] > 0 and open(fly, "rb").read() == pdt.format_frames(fixed)
    assert open(rep).read().split("\n")[:-1] == report_lines(mine, info)
    # -Q without -b, without -W, and for demodARGOS: the usage line, exit status 1, no file
    for prog, args in (("demodPOES", ["-W", fly + "x", "-Q", rep + "x", CLIP_WAV]), ("demodPOES", ["-Q", rep + "x", CLIP_WAV]),
                       ("demodPOES", ["-b", "-Q", rep + "x", CLIP_WAV]), ("demodARGOS", ["-Q", rep + "x", CLIP_WAV])):
        r = subprocess.run([os.path.join(BIN, prog)] + args + ["-o", out + "x"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and ("-Q needs demodPOES with -b -W" in r.stdout or "-b needs demodARGOS with -A, or demodPOES with -W" in r.stdout), args
        assert not os.path.exists(rep + "x") and not os.path.exists(fly + "x"), args
