"""The subcommutated bytes of TIP minor frames on the GPU: the kernels k_subcom_mark, k_subcom_count, k_subcom_scan,
k_subcom_place and k_subcom_spikes against the host restatement, as whole byte strings of samples, offsets and summary -- on every
hand-made case of tests/tip_subcom_cases.py, on three tiles of records with samples, spikes and the two-entry channel on the seams, on
1 200 records under both built-in tables and a table of 256 entries; pdt_tip_subcom behind the chain on the real recording and on its
feed-forward frames; states and arguments; a context's other results untouched; the command line's -E and -H."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tip_dcs_cases as dc
import tip_subcom_cases as sc
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
    return sc.hand_cases(pdt)


@pytest.fixture(scope="module")
def seams(pdt):
    return sc.seam_cases(pdt, pdt.tip_subcom_tile())


@pytest.fixture(scope="module")
def big(pdt):
    return sc.kind4_records(pdt, 1200, flips=1500)


def both(pdt, poes, c, **kw):
    args = (c["frames"], c["table"], c["trusted_only"], c["thr"])
    return poes.tip_subcom_records(*args, **kw), pdt.host_tip_subcom(*args, **kw)


def channel(got, c):
    return got[0][int(got[2][c]):int(got[2][c + 1])]


@pytest.mark.parametrize("k", range(len(sc.HAND_NAMES)))
def test_kernels_equal_host_on_the_hand_made_cases(pdt, poes, hand, k):
    got, want = both(pdt, poes, hand[k])
    assert sc.same(got, want), hand[k]["name"]


@pytest.mark.parametrize("k", range(len(sc.SEAM_NAMES)))
def test_kernels_equal_host_on_tile_seams(pdt, poes, seams, k):
    c = seams[k]
    got, want = both(pdt, poes, c)
    assert sc.same(got, want), c["name"]
    assert len(c["frames"]) == 3 * pdt.tip_subcom_tile() and want[3]["spikes"] >= 1


def test_the_seam_cases_put_samples_where_they_say(pdt, seams):
    T = pdt.tip_subcom_tile()
    res = {c["name"]: pdt.host_tip_subcom(c["frames"], c["table"]) for c in seams}

    def spikes(name):
        s = channel(res[name], 0)
        return s["frame"][(s["flags"] & 8) != 0].tolist()

    # the spike test's neighbours straddle the seams
    assert spikes("spike-left-of-seam") == [T - 1, 2 * T - 1] and spikes("spike-right-of-seam") == [T, 2 * T]
    assert spikes("spikes-on-both-sides") == [T - 1, T, 2 * T - 1, 2 * T]
    # the last record of every tile fires the two-entry channel, entry 1 (byte 41) before entry 2 (byte 40)
    for name in ("spike-left-of-seam", "spikes-on-both-sides"):
        s = channel(res[name], 2)
        assert s["frame"].tolist() == [T - 1, T - 1, 2 * T - 1, 2 * T - 1, 3 * T - 1, 3 * T - 1] and s["entry"].tolist() == [1, 2] * 3
        assert len(channel(res[name], 1)) == 0 and len(channel(res[name], 0)) == 3 * T
    # a tile that gives nothing: the neighbours of the sample in front of it lie a whole tile apart
    sm = res["tile-without-usable-records"][3]
    assert (sm["used"], sm["skipped"], sm["bad_id"]) == (2 * T, T, 0) and spikes("tile-without-usable-records") == [T - 1]
    assert channel(res["tile-without-usable-records"], 2)["frame"].tolist() == [T - 1, T - 1, 3 * T - 1, 3 * T - 1]
    sm = res["tile-of-bad-ids"][3]
    assert (sm["used"], sm["skipped"], sm["bad_id"]) == (2 * T, 0, T) and spikes("tile-of-bad-ids") == [2 * T]
    sm = res["all-at-once"][3]
    assert sm["skipped"] == 8 and sm["byte_parity"] >= 2 and sm["id_parity"] >= 3 and spikes("all-at-once") == [T - 1, T, 2 * T]


def test_seam_cases_with_trusted_only(pdt, poes, seams):
    c = dict(seams[-1], trusted_only=True)
    got, want = both(pdt, poes, c)
    assert sc.same(got, want) and want[3]["dropped"] >= 3 and want[3]["byte_parity"] == want[3]["id_parity"] == 0


def test_1200_records_under_the_built_in_tables(pdt, poes, big):
    for which, nchan in ((pdt.SUBCOM_SEM, 60), (pdt.SUBCOM_HK, 5)):
        for trusted in (False, True):
            got, want = poes.tip_subcom_records(big, which, trusted), pdt.host_tip_subcom(big, which, trusted)
            assert sc.same(got, want), (which, trusted)
            a, n, off, sm = got
            assert sm["used"] == 1200 and sm["channels_hit"] == nchan and len(off) == nchan + 1
            if not trusted:
                # (bytes 20 and 21 lie in group 1, 11 and 14 in group 0: none is uncovered)
                assert set(a["flags"].tolist()) >= ({0, 1, 2, 3, 8} if which == pdt.SUBCOM_SEM else {0, 3, 8}) and not (a["flags"] & 4).any()
                assert n == sum(sum(1 for k in range(1200) if (k % 320) % int(e["period"]) == int(e["phase"])) for e in pdt.subcom_table(which))
    # the bytes are hashed: of two neighbours of a full-byte channel each lies more than 20 away with probability about 0.85, so about
    # 0.7 of the inner samples spike; the four nibble channels (values 0 .. 15) never do.  A good share: a third of all samples
    a, n, off, sm = pdt.host_tip_subcom(big, pdt.SUBCOM_SEM)
    assert sm["spikes"] * 3 > sm["samples"] and not (channel((a, n, off, sm), 30)["flags"] & 8).any()


def test_1200_records_under_a_table_of_256_entries(pdt, poes, big):
    tab = sc.big_table(pdt)
    assert len(tab) == 256 and int(tab["channel"].max()) == 127 and (np.bincount(tab["channel"]) == 2).all()
    for trusted in (False, True):
        got, want = poes.tip_subcom_records(big, tab, trusted, cap=1 << 20), pdt.host_tip_subcom(big, tab, trusted, cap=1 << 20)
        assert sc.same(got, want), trusted
    a, n, off, sm = pdt.host_tip_subcom(big, tab, cap=1 << 20)
    assert n > 40000 and len(a) == n and sm["channels_hit"] == 128 and n > 18 * 64 * 30          # (18 tiles and more, 30 and more samples a record)
    seen = set(a["flags"].tolist())
    assert all(any(f & bit for f in seen) for bit in (1, 2, 4, 8)) and 0 in seen and sm["spikes"] > 1000
    # a cap in the middle of a channel, and one that cuts the count in a tile's middle
    for cap in (int(off[64]) + 3, 1000):
        assert sc.same(poes.tip_subcom_records(big, tab, cap=cap), pdt.host_tip_subcom(big, tab, cap=cap))


def test_cap_and_count(pdt, poes, hand):
    c = [c for c in hand if c["name"] == "own-table"][0]
    full = pdt.host_tip_subcom(c["frames"], c["table"])
    for cap in (0, 1, int(full[2][3]) + 5, full[1], full[1] + 9):
        got, want = both(pdt, poes, c, cap=cap)
        assert sc.same(got, want) and got[1] == full[1] and got[3] == full[3]
    c = [c for c in hand if c["name"] == "spike"][0]
    a, n, off, sm = poes.tip_subcom_records(c["frames"], c["table"], cap=3)
    assert a["flags"].tolist() == [0, 0, 8] and sm["spikes"] == 2 and n == 10
    out, count, s = np.full(4 * 24, 0x55, dtype=np.uint8).view(pdt.SUBCOM_SAMPLE_DTYPE), C.c_int(0), pdt.SubcomSummary()
    fr, t = c["frames"], c["table"]
    assert pdt.lib().pdt_tip_subcom_records(poes._h, fr.ctypes.data, len(fr), t.ctypes.data, len(t), None, out.ctypes.data, 3, C.byref(count), None, C.byref(s)) == 0
    assert count.value == 10 and out[:3].tobytes() == a.tobytes() and out[3].tobytes() == b"\x55" * 24


def test_real_recording_through_the_chain(pdt, clip):
    rate, iq = clip
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        d.demod(iq)
        fr = d.frames_array()
        sem, hk = d.tip_subcom(pdt.SUBCOM_SEM), d.tip_subcom(pdt.SUBCOM_HK)
        assert sc.same(sem, pdt.host_tip_subcom(fr, pdt.SUBCOM_SEM)) and sc.same(sem, d.tip_subcom_records(fr, pdt.SUBCOM_SEM))
        assert sc.same(hk, pdt.host_tip_subcom(fr, pdt.SUBCOM_HK))
    a, n, off, sm = sem
    # (the chain's 48th frame is cut off by the capture's end: skipped)
    assert n == 95 and sm == dict(used=47, skipped=1, bad_id=0, samples=95, dropped=0, byte_parity=0, id_parity=0, spikes=0, channels_hit=44)
    value = lambda name: channel(sem, sc.SEM_NAMES.index(name))["value"].tolist()
    assert value("9E1") == [71, 73] and value("9E2") == [31, 34] and value("3EM") == [13, 13, 13] and value("0EFH") == [0, 0, 34]
    a, n, off, sm = hk
    assert n == 3 and a["channel"].tolist() == [0, 1, 2] and a["value"].tolist() == [0, 174, 175] and a["minor_id"].tolist() == [288, 290, 280]
    assert "%.5f" % float(fr["time"][int(a[0]["frame"])]) == "1.58163"
    # the same samples as the committed text's frames give on the host, but for the times' last digits
    text = pdt.host_tip_subcom(dc.golden_records(pdt), pdt.SUBCOM_SEM)[0]
    for k in ("frame", "minor_id", "channel", "entry", "value", "raw", "flags"):
        assert sem[0][k].tolist() == text[k].tolist()


def test_real_recording_through_the_feed_forward_frames(pdt, poes, clip):
    """The feed-forward path places two more frames in front of the chain's 47 (counters 273 and 274): the chain's 95 SEM samples come back
    with their frame indices moved by two, and what the two frames add is printed"""
    rate, iq = clip
    fr = poes.stage_ffp_frames(rate, iq.astype(np.float32) / np.float32(32768.0))
    got = poes.tip_subcom_records(fr, pdt.SUBCOM_SEM)
    assert sc.same(got, pdt.host_tip_subcom(fr, pdt.SUBCOM_SEM)) and len(fr) == 49
    a, n, off, sm = got
    text = pdt.host_tip_subcom(dc.golden_records(pdt), pdt.SUBCOM_SEM)[0]
    extra = a[a["frame"] < 2]
    print(f"{len(fr)} records, {n} samples, {len(extra)} from the two frames in front: {pdt.format_subcom(extra, pdt.SUBCOM_SEM).decode()}")
    rest = a[a["frame"] >= 2]
    assert len(rest) == 95 and sm["used"] == 49
    for k in ("minor_id", "channel", "entry", "value", "raw"):
        assert rest[k].tolist() == text[k].tolist()
    assert (rest["frame"] - 2).tolist() == text["frame"].tolist() and extra["minor_id"].tolist() and set(extra["minor_id"].tolist()) <= {273, 274}
    assert sc.same(poes.tip_subcom_records(fr, pdt.SUBCOM_HK), pdt.host_tip_subcom(fr, pdt.SUBCOM_HK))


def test_errors_and_states(pdt, hand, clip):
    c = [c for c in hand if c["name"] == "own-table"][0]
    fr, tab = c["frames"], c["table"]
    L = pdt.lib()
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_subcom()                                                      # nothing demodulated yet
        assert sc.same(d.tip_subcom_records(fr, tab), pdt.host_tip_subcom(fr, tab))   # ... the records entry needs nothing
        out, count, sm, off = np.zeros(256, pdt.SUBCOM_SAMPLE_DTYPE), C.c_int(0), pdt.SubcomSummary(), np.zeros(129, np.uint64)

        def rec(frames=fr.ctypes.data, n=len(fr), t=tab, nt=None, cfg=None, o=out.ctypes.data, cap=256, cn=C.byref(count), of=off.ctypes.data, s=C.byref(sm)):
            return L.pdt_tip_subcom_records(d._h, frames, n, t.ctypes.data if t is not None else None, len(t) if nt is None else nt, cfg, o, cap, cn, of, s)

        assert rec() == 0 and rec(of=None) == 0
        assert rec(frames=None) == -1 and rec(n=1 << 31) == -1 and rec(o=None) == -1 and rec(cap=-1) == -1 and rec(cn=None) == -1 and rec(s=None) == -1
        assert rec(t=None, nt=1) == -1 and rec(nt=0) == -1 and rec(cfg=C.byref(pdt.SubcomCfg(0, 256))) == -1 and rec(cfg=C.byref(pdt.SubcomCfg(1, 255))) == 0
        assert rec(t=sc.table(pdt, [(0, 104, 1, 0, 255, 0, 0)])) == -1 and rec(t=sc.table(pdt, [(0, 0, 3, 0, 255, 0, 0)])) == -1
        assert rec(t=sc.table(pdt, [(128, 0, 1, 0, 255, 0, 0)])) == -1 and rec(t=sc.table(pdt, [(0, 0, 1, 0, 0, 0, 0)])) == -1
        assert rec(n=1 << 30, t=sc.table(pdt, [(0, 0, 1, 0, 255, 0, 0)] * 3)) == -1
        assert rec(frames=None, n=0, o=None, cap=0) == 0 and count.value == 0 and sm.samples == 0 and not off[:7].any()
        assert L.pdt_tip_subcom(d._h, tab.ctypes.data, len(tab), C.byref(pdt.SubcomCfg(0, 256)), out.ctypes.data, 8, C.byref(count), None, C.byref(sm)) == -1
        assert L.pdt_tip_subcom(d._h, tab.ctypes.data, len(tab), None, None, 8, C.byref(count), None, C.byref(sm)) == -1
        assert L.pdt_tip_subcom(d._h, None, 0, None, out.ctypes.data, 8, C.byref(count), None, C.byref(sm)) == -1
        d.stream_begin()
        d.stream_push(clip[1][:20000])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_subcom()                                                      # an open stream
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.tip_subcom_records(fr, tab)
        d.stream_end()
    with pdt.Demodulator(pdt.MODE_ARGOS, 51200) as argos:
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.tip_subcom()                                                  # an ARGOS context
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.tip_subcom_records(fr, tab)


def test_nothing_else_of_the_context_changes(pdt, clip, hand):
    rate, iq = clip
    names = ("k_subcom_mark", "k_subcom_count", "k_subcom_scan", "k_subcom_place", "k_subcom_spikes")
    with pdt.Demodulator(pdt.MODE_POES, rate, profile=True) as d:
        d.demod(iq)
        assert not any(k.startswith("k_subcom_") for k in d.kernel_times())

        def state():
            s = d.stats()
            check, tip = d.tip_check()                                   # (the summary, and pdt_tip_frames' records)
            return (d.text(), d.frames_array().tobytes(), d.stage(pdt.ST_BITS).tobytes(), (s.samples, s.symbols, s.bits, s.frames, s.lock_sample), check,
                    tip.tobytes(), d.tip_sync().tobytes(), d.tip_dcs()[0].tobytes())

        before = state()
        got = d.tip_subcom()
        assert state() == before and got[1] == 95
        times = d.kernel_times()
        assert all(times[k][0] == 1 and times[k][1] >= 0 for k in names)
        d.tip_subcom_records(hand[3]["frames"], hand[3]["table"])
        assert state() == before and sc.same(d.tip_subcom(), got) and sc.same(d.tip_subcom(pdt.SUBCOM_HK), pdt.host_tip_subcom(d.frames_array(), pdt.SUBCOM_HK))


def test_command_line(pdt, clip, tmp_path):
    exe = os.path.join(BIN, "demodPOES")
    out, sem, hk, fly, dcs = (str(tmp_path / n) for n in ("minor.txt", "sem.txt", "hk.txt", "fly.txt", "dcs.txt"))
    r = subprocess.run([exe, "-E", sem, "-H", hk, "-C", dcs, "-q", "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:                          # (the API's samples: their times are the chain's, not the text's five decimals)
        d.demod(clip[1])
        a, h = d.tip_subcom(pdt.SUBCOM_SEM)[0], d.tip_subcom(pdt.SUBCOM_HK)[0]
        fw = d.tip_sync()
        b, g = d.tip_subcom_records(fw, pdt.SUBCOM_SEM)[0], d.tip_subcom_records(fw, pdt.SUBCOM_HK)[0]
    assert open(sem, "rb").read() == pdt.format_subcom(a, pdt.SUBCOM_SEM) == sc.format_py(a, sc.SEM_NAMES) and len(a) == 95
    assert open(hk, "rb").read() == pdt.format_subcom(h, pdt.SUBCOM_HK) and len(h) == 3 and os.path.getsize(dcs) > 0
    assert f"SEM samples: 95 in 44 channels, 0 byte parity, 0 counter parity, 0 spikes -> {sem}" in r.stdout
    assert f"Housekeeping samples: 3 in 3 channels, 0 byte parity, 0 counter parity, 0 spikes -> {hk}" in r.stdout
    # with -W the samples are those of the flywheel's records
    r = subprocess.run([exe, "-W", fly, "-E", sem, "-H", hk, "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert len(b) >= 95 and open(sem, "rb").read() == pdt.format_subcom(b, pdt.SUBCOM_SEM) and open(hk, "rb").read() == pdt.format_subcom(g, pdt.SUBCOM_HK)
    # ... and of the feed-forward frames after their repair
    r = subprocess.run([exe, "-b", "-W", fly, "-Q", str(tmp_path / "rep.txt"), "-E", sem, "-o", out, CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SEM samples: " in r.stdout and len(open(sem, "rb").read().split(b"\n")) >= 96, r.stdout[-2000:]
    # a run without frames: empty files
    quiet = str(tmp_path / "quiet.wav")
    hdr = bytearray(open(CLIP_WAV, "rb").read(44))
    x = (np.random.default_rng(5).integers(-300, 300, (50000, 2))).astype("<i2")
    hdr[4:8], hdr[40:44] = (x.nbytes + 36).to_bytes(4, "little"), x.nbytes.to_bytes(4, "little")
    open(quiet, "wb").write(bytes(hdr) + x.tobytes())
    r = subprocess.run([exe, "-E", sem, "-H", hk, "-o", out, quiet], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(sem, "rb").read() == b"" and open(hk, "rb").read() == b"" and "SEM samples: 0 in 0 channels" in r.stdout, r.stdout[-2000:]
    # demodARGOS refuses them
    for opt in ("-E", "-H"):
        r = subprocess.run([os.path.join(BIN, "demodARGOS"), opt, sem + "x", "-o", out + "x", CLIP_WAV], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and f"{opt} needs demodPOES" in r.stdout and not os.path.exists(sem + "x")
