"""The DCS-2 platform messages in TIP minor frames on the GPU: the kernels k_dcs_gather, k_dcs_maps, k_dcs_scan and k_dcs_pack
against the host restatement, exact in every field and in the summary, the time included -- on every hand-made stream of
tests/tip_dcs_cases.py, on the streams that put packets, shadowed heads and segment breaks on tile seams, on 1 200 records in one segment;
pdt_tip_dcs behind the chain on the real recording and on a synthetic capture that carries DCS packets; the feed-forward frames of the
real recording; states and arguments; a context's other results untouched; the command line's -C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tip_dcs_cases as dc
from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
CLIP_WAV = os.path.join(ROOT, "tests", "golden", "5sec_clip.wav")


@pytest.fixture(scope="module")
def poes(pdt):
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        yield d


@pytest.fixture(scope="module")
def hand(pdt):
    return dc.hand_cases(pdt)


@pytest.fixture(scope="module")
def seams(pdt):
    return dc.seam_cases(pdt, pdt.tip_dcs_tile())


@pytest.fixture(scope="module")
def clip_packets(pdt):
    return pdt.host_tip_dcs(dc.golden_records(pdt))


@pytest.mark.parametrize("k", range(len(dc.HAND_NAMES)))
def test_kernels_equal_host_on_the_hand_made_streams(pdt, poes, hand, k):
    c = hand[k]
    assert dc.same(poes.tip_dcs_records(c["frames"], c["channel_max"]), pdt.host_tip_dcs(c["frames"], c["channel_max"])), c["name"]


@pytest.mark.parametrize("k", range(14))
def test_kernels_equal_host_on_tile_seams(pdt, poes, seams, k):
    c = seams[k]
    got, want = poes.tip_dcs_records(c["frames"]), pdt.host_tip_dcs(c["frames"])
    assert dc.same(got, want), c["name"]
    assert want[1] > 30 and len(c["frames"]) == 3 * pdt.tip_dcs_tile() // 32


def test_the_seam_streams_put_heads_where_they_say(pdt, seams):
    T = pdt.tip_dcs_tile()
    at = {c["name"]: set(pdt.host_tip_dcs(c["frames"])[0]["stream_index"].tolist()) for c in seams}
    for d in (-2, -1, 0, 1):
        assert {T + d, 2 * T + d} <= at[f"head-at-seam{d:+d}"]
    assert {T - 43, 2 * T - 15} <= at["one-byte-across"] and {T - 1, T + 43, 2 * T - 1} <= at["43-bytes-across"]
    assert T - 10 in at["shadowed-head-first-in-tile"] and T not in at["shadowed-head-first-in-tile"] and T + 34 in at["shadowed-head-first-in-tile"]
    assert T - 1 not in at["break-on-seam-head-1"] and T in at["break-on-seam-head+0"] and T + 1 in at["break-on-seam-head+1"]


def test_many_tiles_in_one_segment(pdt, poes):
    p = pdt.synth_params(4, 50000, 1000.0, 7)
    fr = dc.kind4_records(pdt, p, 1200)
    got, want = poes.tip_dcs_records(fr), pdt.host_tip_dcs(fr)
    assert dc.same(got, want)
    sm = got[2]
    assert (got[1], sm["segments"], sm["used"], sm["complete"], sm["doppler_bad"]) == (1200, 1, 1200, 1200, 0) and 1200 * 32 > 18 * pdt.tip_dcs_tile()


def test_cap_and_count(pdt, poes, hand):
    fr = [c for c in hand if c["name"] == "back-to-back"][0]["frames"]
    full = pdt.host_tip_dcs(fr)
    for cap in (0, 1, 3, 4, 9):
        assert dc.same(poes.tip_dcs_records(fr, cap=cap), pdt.host_tip_dcs(fr, cap=cap))
    a, n, sm = poes.tip_dcs_records(fr, cap=0)
    assert (len(a), n, sm) == (0, 4, full[2])
    out, count, s = np.full(3 * 88, 0x55, dtype=np.uint8).view(pdt.DCS_PACKET_DTYPE), C.c_int(0), pdt.DcsSummary()
    assert pdt.lib().pdt_tip_dcs_records(poes._h, fr.ctypes.data, len(fr), None, out.ctypes.data, 2, C.byref(count), C.byref(s)) == 0 and count.value == 4
    assert out[:2].tobytes() == full[0][:2].tobytes() and out[2].tobytes() == b"\x55" * 88


def test_real_recording_through_the_chain(pdt, clip, clip_packets):
    rate, iq = clip
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        d.demod(iq)
        got = d.tip_dcs()
        fr = d.frames_array()
        assert dc.same(got, pdt.host_tip_dcs(fr)) and dc.same(got, d.tip_dcs_records(fr))
    a, n, sm = got
    assert n == 25 and a["stream_index"].tolist() == dc.CLIP_INDICES and a["bytes"].tobytes() == clip_packets[0]["bytes"].tobytes()
    assert (sm["used"], sm["skipped"], sm["segments"], sm["complete"], sm["doppler_bad"], sm["shadowed"], sm["bad_code"]) == (47, 1, 1, 24, 0, 0, 0)
    assert (int(a[0]["channel"]), int(a[0]["nbytes"]), int(a[0]["time_code"]), int(a[0]["id"]), int(a[0]["doppler_raw"]) / 32) == (7, 28, 1510879, 0x9FAD2098, 881.0625)
    assert (int(a[11]["nbytes"]), int(a[11]["id"]), int(a[24]["nbytes"])) == (44, 0x07D7B0D4, 9)


def test_real_recording_through_the_feed_forward_frames(pdt, poes, clip, clip_packets):
    """The feed-forward path places two more frames in front of the chain's 47: the 25 packets come back 64 stream bytes later, and what
    the two frames add is printed.  Seen when this was written: 49 records, 26 packets -- one more complete packet in front, 44 bytes,
    channel 2, time code 1510830, ID D3CEA05F, even Doppler parity."""
    rate, iq = clip
    fr = poes.stage_ffp_frames(rate, iq.astype(np.float32) / np.float32(32768.0))
    got = poes.tip_dcs_records(fr)
    assert dc.same(got, pdt.host_tip_dcs(fr)) and len(fr) == 49
    a, n, sm = got
    extra = n - 25
    print(f"{len(fr)} records, {n} packets, {extra} in front of the chain's first: {pdt.format_dcs_packets(a[:max(extra, 0)]).decode()}")
    assert extra >= 0 and a["stream_index"][extra:].tolist() == [k + 64 for k in dc.CLIP_INDICES]
    assert a["bytes"][extra:].tobytes() == clip_packets[0]["bytes"].tobytes() and a["nbytes"][extra:].tolist() == clip_packets[0]["nbytes"].tolist()
    assert (a["stream_index"][:extra] < 64 + 12).all() and sm["segments"] == 1 and sm["used"] == 49


def test_kind_4_capture_through_the_chain(pdt):
    p = pdt.synth_params(4, 50000, 1000.0, 7)
    x = pdt.synth_capture(4, 50000, 2.0, seed=7)
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        d.demod(x)
        fr = d.frames_array()
        got = d.tip_dcs()
    assert dc.same(got, pdt.host_tip_dcs(fr))
    a, n, sm = got
    ok = fr[(fr["complete"] == 1) & (fr["nbytes"] == 104)]
    number = [(int(b[4]) & 1) << 8 | int(b[5]) for b in ok["bytes"]]                       # the minor-frame counter = the frame's number (under 320)
    # (2 s are 20 frames; the loop needs a few of them to lock: at least 12 decoded frames hold at least 5 whole slot groups, 10 packets)
    assert len(ok) >= 12 and number == list(range(number[0], number[0] + len(ok))) and sm["segments"] == 1
    assert all(bytes(b) == bytes(pdt.synth_poes_frame(p, k)) for b, k in zip(ok["bytes"], number))
    lo, hi = 32 * number[0], 32 * (number[-1] + 1)                                           # the stream bytes the decoded frames hold
    sent = 0
    found = {int(r["stream_index"]) + lo: r for r in a}
    for s in range(lo // 64, hi // 64 + 1):
        ta, tb = pdt.synth_dcs_packet(p, s, 0), pdt.synth_dcs_packet(p, s, 1)
        for which, truth, q in ((0, ta, 64 * s), (1, tb, 64 * s + len(ta))):
            if q < lo or q + len(truth) > hi:
                continue
            sent += 1
            r = found[q]
            assert bytes(r["bytes"][:len(truth)]) == bytes(truth) and int(r["complete"]) == 1 and int(r["doppler_ok"]) == 1
            assert int(r["time_code"]) == 2 * s + which and int(r["channel"]) == (s + 3 * which) % 8
    print(f"{len(ok)} decoded frames ({number[0]} .. {number[-1]}), {sent} transmitted packets inside them, {n} found")
    assert sent >= 10 and sm["complete"] == sent and sm["doppler_bad"] == 0


def test_errors_and_states(pdt, hand, clip):
    fr = hand[0]["frames"]
    L = pdt.lib()
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_dcs()                                                         # nothing demodulated yet
        assert dc.same(d.tip_dcs_records(fr), pdt.host_tip_dcs(fr))               # ... the records entry needs nothing
        out, count, sm = np.zeros(8, pdt.DCS_PACKET_DTYPE), C.c_int(0), pdt.DcsSummary()
        o, c, s = out.ctypes.data, C.byref(count), C.byref(sm)
        assert L.pdt_tip_dcs_records(d._h, None, 1, None, o, 8, c, s) == -1 and L.pdt_tip_dcs_records(d._h, fr.ctypes.data, 1 << 31, None, o, 8, c, s) == -1
        assert L.pdt_tip_dcs_records(d._h, fr.ctypes.data, 1, None, None, 8, c, s) == -1 and L.pdt_tip_dcs_records(d._h, fr.ctypes.data, 1, None, o, -1, c, s) == -1
        assert L.pdt_tip_dcs_records(d._h, fr.ctypes.data, 1, None, o, 8, None, s) == -1 and L.pdt_tip_dcs_records(d._h, fr.ctypes.data, 1, None, o, 8, c, None) == -1
        assert L.pdt_tip_dcs_records(d._h, fr.ctypes.data, 1, C.byref(pdt.DcsCfg(17, 0)), o, 8, c, s) == -1
        assert L.pdt_tip_dcs(d._h, C.byref(pdt.DcsCfg(17, 0)), o, 8, c, s) == -1 and L.pdt_tip_dcs(d._h, None, None, 8, c, s) == -1
        assert L.pdt_tip_dcs_records(d._h, None, 0, None, None, 0, c, s) == 0 and count.value == 0 and sm.packets == 0
        d.stream_begin()
        d.stream_push(clip[1][:20000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_dcs()                                                         # an open stream
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_dcs_records(fr)
        d.stream_end()
    with pdt.Demodulator(pdt.MODE_ARGOS, 51200) as argos:
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.tip_dcs()                                                     # an ARGOS context
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.tip_dcs_records(fr)


def test_nothing_else_of_the_context_changes(pdt, clip, hand):
    rate, iq = clip
    with pdt.Demodulator(pdt.MODE_POES, rate, profile=True) as d:
        d.demod(iq)
        assert not any(k.startswith("k_dcs_") for k in d.kernel_times())

        def state():
            s = d.stats()
            return (d.text(), d.frames_array().tobytes(), d.stage(pdt.ST_BITS).tobytes(), (s.samples, s.symbols, s.bits, s.frames, s.lock_sample), str(d.tip_check()))

        before = state()
        got = d.tip_dcs()
        assert state() == before and got[1] == 25
        times = d.kernel_times()
        assert all(times[k][0] == 1 and times[k][1] >= 0 for k in ("k_dcs_gather", "k_dcs_maps", "k_dcs_scan", "k_dcs_pack"))
        d.tip_dcs_records(hand[0]["frames"])
        assert state() == before and dc.same(d.tip_dcs(), got)


def id_table(packets):
    ids = {}
    for r in packets:
        ids[int(r["id"])] = ids.get(int(r["id"]), 0) + 1
    return "".join("%08X %u\n" % (i, c) for i, c in sorted(ids.items(), key=lambda v: (-v[1], v[0]))).encode()


def test_command_line(pdt, poes, clip, clip_packets, tmp_path):
    exe = os.path.join(BIN, "demodPOES")
    out, dcs, fly = str(tmp_path / "minor.txt"), str(tmp_path / "dcs.txt"), str(tmp_path / "fly.txt")
    r = subprocess.run([exe, "-C", dcs, "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:                          # (the API's packets: their times are the chain's, not the text's five decimals)
        d.demod(clip[1])
        a = d.tip_dcs()[0]
        b = d.tip_dcs_records(d.tip_sync())[0]
    assert a["bytes"].tobytes() == clip_packets[0]["bytes"].tobytes()
    assert open(dcs, "rb").read() == pdt.format_dcs_packets(a) + b"\n" + id_table(a)
    assert f"DCS packets: 25, 24 complete, 0 Doppler parity failures, 1 segments -> {dcs}" in r.stdout
    # with -W the packets are those of the flywheel's records
    r = subprocess.run([exe, "-W", fly, "-C", dcs, "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert len(b) >= 25 and open(dcs, "rb").read() == pdt.format_dcs_packets(b) + b"\n" + id_table(b)
    # a run without frames: an empty file
    quiet = str(tmp_path / "quiet.wav")
    hdr = bytearray(open(CLIP_WAV, "rb").read(44))
    x = (np.random.default_rng(5).integers(-300, 300, (50000, 2))).astype("<i2")
    hdr[4:8], hdr[40:44] = (x.nbytes + 36).to_bytes(4, "little"), x.nbytes.to_bytes(4, "little")
    open(quiet, "wb").write(bytes(hdr) + x.tobytes())
    r = subprocess.run([exe, "-C", dcs, "-o", out, quiet], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(dcs, "rb").read() == b"" and "DCS packets: 0, 0 complete" in r.stdout, r.stdout[-2000:]
    # demodARGOS refuses -C
    r = subprocess.run([os.path.join(BIN, "demodARGOS"), "-C", dcs + "x", "-o", out + "x", CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "-C needs demodPOES" in r.stdout and not os.path.exists(dcs + "x")
