"""The feed-forward POES bits on the GPU: the four kernels against the host restatement byte for byte -- record, bits, the
soft values' bit patterns, sample indices, the per-block table -- on every stream of tests/ffp_cases.py and on streams that sit on the
seams of the kernels' own tiling; the frames of pdt_stage_ffp_frames against pdt_host_tip_sync on the same bits, on the weak capture
and the real recording; a context's channel stream, its other results untouched; states, arguments, kernel names; the command line."""
import os
import subprocess

import numpy as np
import pytest

import ffp_cases as fc
from conftest import ROOT
from test_gpu_bursts import STAT_FIELDS
from test_tip_sync import weak_capture

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
CLIP_WAV = os.path.join(ROOT, "tests", "golden", "5sec_clip.wav")
KERNELS = ("k_ffp_mix", "k_ffp_search", "k_ffp_track", "k_ffp_bits")
MIX_TILE = 1024                                 # samples one workgroup of k_ffp_mix takes (FFP_MIX_TILE)


@pytest.fixture(scope="module")
def poes(pdt):
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        yield d


def same(pdt, d, fs, y, **cfg):
    got, want = d.stage_ffp_bits(fs, y, **cfg), pdt.host_ffp_bits(fs, y, **cfg)
    assert fc.same_bits(got, want), (cfg, got.sync, want.sync, fc.blocks_of(got)[:8], fc.blocks_of(want)[:8])
    return got


@pytest.mark.parametrize("name", [c[0] for c in fc.cases() + fc.tone_cases()])
def test_stage_equals_host_on_every_cpu_case(pdt, poes, name):
    _, fs, y, cfg = [c for c in fc.cases() + fc.tone_cases() if c[0] == name][0]
    same(pdt, poes, fs, y, **cfg)


def seam_cases():
    out = []
    # k_ffp_mix: exactly one workgroup's samples, and one fewer and one more
    for n in (MIX_TILE - 1, MIX_TILE, MIX_TILE + 1):
        out.append((f"mix-tile-{n}", 49920, fc.stream(49920, n), dict(residual_hz=40.0, **fc.SMALL)))
    # a tone-segment seam (sample 4096) in the middle of a block's halo: B = 69 at 50 ksps is L = 415, block 10 starts at sample 4150 and
    # its reference window reaches 17 bits = 102 samples back
    f = np.where(np.arange(2 * 4096 + 300) < 4096, -3470.0, -3500.0)
    out.append(("tone-seam-in-a-halo", 50000, fc.stream(50000, len(f), carrier_hz=f, noise=0.01), dict(block_bits=69, clock_steps=8, smooth_blocks=1)))
    # the smallest and largest stagings at 250 ksps: B = 832 with W = 64 takes several chunks of a block and several groups of hypotheses
    out.append(("250k-B64", 250000, fc.stream(250000, 3 * fc.block_len(64, 250000) + 11, delay=7.0), dict(residual_hz=40.0, block_bits=64)))
    out.append(("250k-B832", 250000, fc.stream(250000, 2 * fc.block_len(832, 250000) + 1234, delay=7.0), dict(residual_hz=40.0, block_bits=832)))
    out.append(("250k-B832-W64-T64", 250000, fc.stream(250000, fc.block_len(832, 250000) + 999, delay=7.0),
                dict(residual_hz=40.0, block_bits=832, ref_bits=64, clock_steps=64)))
    # T = 8 and T = 64 at the defaults otherwise; every stream's first block has a halo in front of sample 0 and its last one behind n
    out.append(("T8", 50000, fc.stream(50000, 5000, delay=2.0), dict(residual_hz=40.0, clock_steps=8)))
    out.append(("T64", 50000, fc.stream(50000, 5000, delay=2.0), dict(residual_hz=40.0, clock_steps=64)))
    out.append(("P64-W64", 1064960, fc.stream(1064960, 3 * fc.block_len(64, 1064960) + 5, delay=30.0), dict(residual_hz=40.0, block_bits=64, ref_bits=64)))
    # a long block count: k_ffp_track's lanes take more than one block each
    out.append(("600-blocks", 49920, fc.stream(49920, 600 * 384 + 77, ppm=150.0), dict(residual_hz=40.0, block_bits=64, clock_steps=16)))
    return out


@pytest.mark.parametrize("name", [c[0] for c in seam_cases()])
def test_stage_equals_host_on_the_kernels_seams(pdt, poes, name):
    _, fs, y, cfg = [c for c in seam_cases() if c[0] == name][0]
    got = same(pdt, poes, fs, y, **cfg)
    if name == "600-blocks":
        assert fc.aligned(got.bits) == 0 and int(got.blocks["phi"][-1]) < -5 * 16      # (a fast clock: phi falls, through five whole bits)


def frames_equal_host(pdt, got, fr, info, fs):
    want, winfo = pdt.host_tip_sync(got.bits.tobytes(), with_info=True)
    assert len(fr) == len(want) and info.tobytes() == winfo.tobytes()
    for k in ("bit_index", "inverted", "nbytes", "complete", "pad"):
        assert (fr[k] == want[k]).all(), k
    assert fr["bytes"].tobytes() == want["bytes"].tobytes()
    assert (fr["time_src"] == got.index[fr["bit_index"]]).all() and (fr["time"] == got.index[fr["bit_index"]] / float(fs)).all()
    return len(fr)


def test_frames_on_the_real_recording(pdt, poes, clip):
    rate, iq = clip
    y = iq.astype(np.float32) / np.float32(32768.0)
    fr, info = poes.stage_ffp_frames(rate, y, with_info=True)
    got = poes.ffp_read()
    assert fc.same_bits(got, pdt.host_ffp_bits(rate, y))
    assert frames_equal_host(pdt, got, fr, info, rate) >= 47
    # the strictest triple reaches the library
    strict, sinfo = poes.stage_ffp_frames(rate, y, 0, 1, 2, with_info=True)
    want = pdt.host_tip_sync(got.bits.tobytes(), 0, 1, 2)
    assert (strict["bit_index"] == want["bit_index"]).all() and len(strict) >= 47
    small, found = poes.stage_ffp_frames(rate, y, cap=3, with_count=True)
    assert found == len(fr) and small["bytes"].tobytes() == fr[:3]["bytes"].tobytes()


def test_frames_on_the_weak_capture(pdt, poes):
    p, x = weak_capture(pdt, seconds=6.0)
    y = x.astype(np.float32) / np.float32(32768.0)
    fr, info = poes.stage_ffp_frames(50000, y, with_info=True)
    got = poes.ffp_read()
    assert fc.same_bits(got, pdt.host_ffp_bits(50000, y))
    assert frames_equal_host(pdt, got, fr, info, 50000) > 40


def wideband_clip(clip):
    """the real recording as a capture at twice its rate: every sample twice (a zero-order hold; the down-converter's filter takes the
    image out)"""
    return np.repeat(clip[1], 2, axis=0)


def test_a_contexts_channel_stream_and_nothing_else_changes(pdt, clip):
    x = wideband_clip(clip)
    with pdt.Demodulator(pdt.MODE_POES, 50000, profile=True) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.ffp_bits()                                                      # nothing demodulated yet
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.ffp_read()
        d.set_channel(2, 0.0).demod_channel(x)
        assert not any(k in d.kernel_times() for k in KERNELS)

        def state():
            s = d.stats()
            return (d.text(), d.frames_array().tobytes(), d.stage(pdt.ST_BITS).tobytes(), d.stage(pdt.ST_CHANNEL).tobytes(), d.stage(pdt.ST_AGC).tobytes(),
                    tuple(getattr(s, f) for f in STAT_FIELDS), d.tip_sync().tobytes(), d.tones().tobytes())

        before = state()
        y = d.stage(pdt.ST_CHANNEL)
        sync = d.ffp_bits()
        got = d.ffp_read()
        # (a context's tone search is its mode's PLL range, the host's every bin: the carrier lies inside both)
        want = pdt.host_ffp_bits(50000, y)
        assert fc.same_bits(got, want) and sync.tobytes() == got.sync.tobytes() and int(sync["segs_valid"]) == int(sync["segs"]) > 50
        times = d.kernel_times()
        assert all(times[k][1] >= 0 for k in KERNELS) and [times[k][0] for k in KERNELS] == [1, 1, 2, 1], times
        fr, info = d.ffp_frames(with_info=True)
        assert frames_equal_host(pdt, d.ffp_read(), fr, info, 50000) >= 47
        given = d.ffp_bits(residual_hz=-3480.0, block_bits=104)
        assert int(given["segs"]) == 0 and fc.same_bits(d.ffp_read(), pdt.host_ffp_bits(50000, y, residual_hz=-3480.0, block_bits=104))
        assert state() == before
        # the stage entry leaves the context alone as well
        d.stage_ffp_bits(50000, y[:5000], residual_hz=-3480.0)
        assert state() == before


def test_errors_and_states(pdt, poes, clip):
    y = fc.stream(50000, 3000)
    for bad in (dict(block_bits=63), dict(block_bits=833), dict(clock_steps=7), dict(clock_steps=65), dict(ref_bits=65), dict(ref_bits=-1),
                dict(smooth_blocks=17), dict(smooth_blocks=-1), dict(residual_hz=25000.0), dict(residual_hz=float("nan"))):
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.stage_ffp_bits(50000, y, **bad)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.stage_ffp_frames(50000, y, **bad)
    for rate in (49919, 1064961, 32000):
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.stage_ffp_bits(rate, y)
    for bad in ((4, None, None), (None, 9, None), (None, None, 1)):
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.stage_ffp_frames(50000, y, *bad)
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        poes.stage_ffp_frames(50000, y, cap=-1)
    with pdt.Demodulator(pdt.MODE_ARGOS, 51200) as argos:
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.stage_ffp_bits(51200, y)                                    # an ARGOS context
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.ffp_bits()
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        d.demod(clip[1][:60000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.ffp_bits()                                                      # a plain capture leaves no channel stream
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.ffp_frames()
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.ffp_read()
        got = d.stage_ffp_bits(50000, y, residual_hz=40.0)                    # ... the stage entry needs none
        assert fc.same_bits(got, pdt.host_ffp_bits(50000, y, residual_hz=40.0)) and fc.same_bits(d.ffp_read(), got)
        d.stream_begin()
        d.stream_push(clip[1][:20000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.stage_ffp_bits(50000, y)                                        # an open stream
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.ffp_bits()
        d.stream_end()
    with pdt.Demodulator(pdt.MODE_POES, 32000) as d:
        d.set_channel(2, 0.0).demod_channel(np.zeros((20000, 2), dtype=np.int16))
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            d.ffp_bits()                                                      # a channel rate below 49 920


def test_command_line(pdt, poes, clip, tmp_path):
    exe = os.path.join(BIN, "demodPOES")
    out, fly = str(tmp_path / "minor.txt"), str(tmp_path / "fly.txt")
    golden = open(os.path.join(ROOT, "tests", "golden", "clip.c10000.txt"), "rb").read()
    # a plain I,Q file through the stage entry
    r = subprocess.run([exe, "-q", "-b", "-W", fly, "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert open(out, "rb").read() == golden
    want = poes.stage_ffp_frames(50000, clip[1].astype(np.float32) / np.float32(32768.0))
    assert len(want) >= 47 and open(fly, "rb").read() == pdt.format_frames(want)
    assert f"Flywheel frames: {len(want)} -> " in r.stdout and "Feed-forward bits: " in r.stdout
    sm, _ = poes.tip_check_records(want)
    assert f"Flywheel: {sm['good_frames']} out of {len(want)} Error Free Frames" in r.stdout
    r = subprocess.run([exe, "-b", "-W", fly, "-w", "0,1,2", "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(fly, "rb").read() == pdt.format_frames(poes.stage_ffp_frames(50000, clip[1].astype(np.float32) / np.float32(32768.0), 0, 1, 2))
    # the channel stream of a wideband capture
    wide = str(tmp_path / "wide.wav")
    x = wideband_clip(clip)
    hdr = bytearray(open(CLIP_WAV, "rb").read(44))
    hdr[24:28] = (100000).to_bytes(4, "little")
    hdr[40:44] = (x.nbytes).to_bytes(4, "little")
    open(wide, "wb").write(bytes(hdr) + x.astype("<i2").tobytes())
    r = subprocess.run([exe, "-x", "2", "-t", "0", "-b", "-W", fly, "-o", out, wide], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        d.set_channel(2, 0.0).demod_channel(x)
        want = d.ffp_frames()
    assert len(want) >= 47 and open(fly, "rb").read() == pdt.format_frames(want)
    # refusals, each with the usage line and without a file
    for args in (["-b", CLIP_WAV], ["-b", "-W", fly + "x", "-l", CLIP_WAV], ["-b", "-W", fly + "x", "-f", "10", CLIP_WAV],
                 ["-x", "2", "-t", "0", "-t", "1", "-b", "-W", fly + "x", wide]):
        r = subprocess.run([exe] + args + ["-o", out + "x"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and ("-b needs demodARGOS with -A, or demodPOES with -W" in r.stdout or "-W and -w need demodPOES" in r.stdout), args
        assert not os.path.exists(fly + "x"), args
