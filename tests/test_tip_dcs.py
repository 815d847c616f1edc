"""The DCS-2 platform messages in TIP minor frames without a GPU: pdt_host_tip_dcs against a Python statement of the rule
written from the header's text (tests/tip_dcs_cases.py), field by field and the time bit for bit -- on the hand-made streams, on the
streams that put packets on tile seams, on the real recording (whose 25 packets are written out here) and on the synthesiser's kind 4,
whose transmitted packets all come back; the packets' text against Python's %; every argument error; and the rule's host statement under
AddressSanitizer in a program of its own."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import tip_dcs_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hand(pdt):
    return dc.hand_cases(pdt)


@pytest.fixture(scope="module")
def clip_records(pdt):
    return dc.golden_records(pdt)


@pytest.fixture(scope="module")
def clip_packets(pdt, clip_records):
    return pdt.host_tip_dcs(clip_records)


def by_name(hand, name):
    return [c for c in hand if c["name"] == name][0]


def test_hand_cases_cover_the_list(hand):
    assert [c["name"] for c in hand] == dc.HAND_NAMES


@pytest.mark.parametrize("k", range(len(dc.HAND_NAMES)))
def test_host_equals_the_model(pdt, hand, k):
    c = hand[k]
    got = pdt.host_tip_dcs(c["frames"], c["channel_max"])
    assert dc.same_as_model(got, dc.model(c["frames"], c["channel_max"])), c["name"]
    sm = got[2]
    assert sm["used"] + sm["skipped"] == len(c["frames"]) and sm["heads"] == sm["packets"] + sm["shadowed"] and sm["stream_bytes"] == 32 * sm["used"]


def test_hand_derived_outcomes(pdt, hand):
    def run(name):
        c = by_name(hand, name)
        return pdt.host_tip_dcs(c["frames"], c["channel_max"])

    a, n, sm = run("shadowed")                                   # the pair inside the data is counted and opens nothing; the packet is intact
    assert (n, sm["heads"], sm["shadowed"]) == (2, 3, 1) and a["stream_index"].tolist() == [5, 33] and a["nbytes"].tolist() == [28, 16]
    assert bytes(a[0]["bytes"][12:15]) == b"\xD6\x02\x5A" and a["complete"].tolist() == [1, 1] and a["doppler_ok"].tolist() == [1, 1]
    a, n, sm = run("first-byte")                                 # (the reference's rule never sees the stream's first byte)
    assert n == 1 and (int(a[0]["stream_index"]), int(a[0]["frame"]), int(a[0]["slot"]), int(a[0]["nbytes"])) == (0, 0, 0, 20)
    a, n, sm = run("first-byte-second-segment")
    assert a["stream_index"].tolist() == [0, 64] and a["frame"].tolist() == [0, 2] and sm["segments"] == 2 and int(a[1]["id"]) == 0xFFFFFFFF
    assert run("last-byte")[1] == 0 and run("second-to-last-byte")[1] == 0
    a, n, sm = run("third-to-last-byte")                         # k + 2 is the segment's last byte: a head, three bytes of a packet
    assert n == 1 and (int(a[0]["nbytes"]), int(a[0]["complete"]), int(a[0]["time_code"]), int(a[0]["id"]), int(a[0]["doppler_ok"])) == (3, 0, 0, 0, 0)
    assert [run(f"channels-{cm}")[0]["channel"].tolist() for cm in (0, 8, 9, 16, 1)] == [[7, 0], [7, 0], [7, 8, 0], [7, 8, 9, 0, 15], [0]]
    a, n, sm = run("bad-codes")
    assert (n, sm["bad_code"], sm["heads"]) == (1, 8, 1) and int(a[0]["stream_index"]) == 70
    a, n, sm = run("doppler-flipped")
    assert a["doppler_ok"].tolist() == [0, 1] and sm["doppler_bad"] == 1 and a["complete"].tolist() == [1, 1]
    text = pdt.format_dcs_packets(a).decode().split("\n")
    assert text[0].split()[5].startswith("*") and not text[1].split()[5].startswith("*")
    a, n, sm = run("ineligible-between")
    assert (sm["used"], sm["skipped"], sm["segments"]) == (5, 3, 3) and a["frame"].tolist() == [0, 1, 3, 7]
    assert a["stream_index"].tolist() == [10, 60, 2 * 32 + 120 - 96, 4 * 32 + 2] and a["complete"].tolist() == [1, 0, 0, 1]
    a, n, sm = run("out-of-order")
    # (the records reversed: the one in front holds the packet at 100, the next only the tail of the packet at 60, the third the packet
    # at 40 and the first four bytes of the one at 60, the last the packet at 2)
    assert sm["segments"] == 4 and a["frame"].tolist() == [0, 2, 2, 3] and a["complete"].tolist() == [1, 1, 0, 1] and a["nbytes"].tolist() == [16, 16, 4, 16]
    assert run("no-records")[1:] == (0, dict.fromkeys(dc.SUMMARY, 0))
    a, n, sm = run("back-to-back")
    assert a["stream_index"].tolist() == [0, 44, 60, 104] and a["nbytes"].tolist() == [44, 16, 44, 24] and a["complete"].tolist() == [1, 1, 1, 0]


def test_cap_smaller_than_the_count(pdt, hand):
    c = by_name(hand, "back-to-back")
    full = pdt.host_tip_dcs(c["frames"])
    for cap in (0, 1, 3, 4, 5):
        a, n, sm = pdt.host_tip_dcs(c["frames"], cap=cap)
        assert n == 4 and sm == full[2] and len(a) == min(cap, 4) and a.tobytes() == full[0][:cap].tobytes()
    out, count, sm = np.full(3, 0x55, dtype=np.uint8).repeat(88).view(pdt.DCS_PACKET_DTYPE), C.c_int(0), pdt.DcsSummary()
    fr = c["frames"]
    assert pdt.lib().pdt_host_tip_dcs(fr.ctypes.data, len(fr), None, out.ctypes.data, 2, C.byref(count), C.byref(sm)) == 0 and count.value == 4
    assert out[:2].tobytes() == full[0][:2].tobytes() and out[2].tobytes() == b"\x55" * 88                  # nothing behind cap is written


@pytest.mark.parametrize("k", range(14))
def test_seam_streams_on_the_host(pdt, k):
    c = dc.seam_cases(pdt, pdt.tip_dcs_tile())[k]
    assert dc.same_as_model(pdt.host_tip_dcs(c["frames"]), dc.model(c["frames"])), c["name"]


def test_seam_case_count(pdt):
    T = pdt.tip_dcs_tile()
    assert T == 2048 and len(dc.seam_cases(pdt, T)) == 14


def test_real_recording_the_oracles_frames_are_832_bits_apart(orc, clip, clip_records):
    rate, iq = clip
    o = orc.Oracle(orc.POES, rate, iq)                                     # (the records live as long as it does)
    fr = o.frames()
    assert len(fr) == 48 and not fr[47].complete                           # (the capture ends inside the 48th, which the text shows without a newline)
    fr = fr[:47]
    assert all(f.complete == 1 and f.nbytes == 104 for f in fr)
    assert {fr[k + 1].bit_index - fr[k].bit_index for k in range(46)} == {832}
    assert [bytes(f.bytes) for f in fr] == [bytes(v) for v in clip_records["bytes"]]
    assert ["%.5f" % f.time for f in fr] == ["%.5f" % t for t in clip_records["time"]]


def test_real_recording(pdt, clip_records, clip_packets):
    a, n, sm = clip_packets
    assert dc.same_as_model(clip_packets, dc.model(clip_records))
    assert n == 25 and a["stream_index"].tolist() == dc.CLIP_INDICES
    assert sm == dict(used=47, skipped=0, segments=1, stream_bytes=1504, heads=25, shadowed=0, bad_code=0, packets=25, complete=24, doppler_bad=0)
    assert (int(a[0]["channel"]), int(a[0]["nbytes"]), int(a[0]["time_code"]), int(a[0]["id"]), int(a[0]["doppler_raw"]) / 32) == (7, 28, 1510879, 0x9FAD2098, 881.0625)
    assert (int(a[11]["nbytes"]), int(a[11]["id"])) == (44, 0x07D7B0D4)
    assert (int(a[24]["nbytes"]), int(a[24]["complete"])) == (9, 0) and a["complete"][:24].all() and a["doppler_ok"][:24].all()
    lengths = sorted(set(a["nbytes"][:24].tolist()))
    assert lengths == [16, 20, 24, 28, 32, 36, 40, 44] and a["nbytes"].tolist().count(28) == 1 and a["nbytes"].tolist().count(44) == 1
    # the time is the D6 byte's own: frame time + byte * (0.1 / 104)
    assert float(a[0]["time"]) == float(clip_records["time"][0]) + dc.SLOTS[12] * (0.1 / 104) and (int(a[0]["frame"]), int(a[0]["slot"])) == (0, 12)


def test_real_recording_older_build(pdt, clip_packets):
    """tests/golden/old_build_minorFrame.txt holds 46 of the frames: the same packets without the first"""
    fr = dc.golden_records(pdt, "old_build_minorFrame.txt")
    a, n, sm = pdt.host_tip_dcs(fr)
    assert len(fr) == 46 and n == 24 and a["bytes"].tobytes() == clip_packets[0]["bytes"][1:].tobytes()
    assert a["nbytes"].tolist() == clip_packets[0]["nbytes"][1:].tolist()


def test_real_recording_without_frame_20(pdt, clip_records, clip_packets):
    """Frame 20's slots are stream bytes 640 .. 671: the packet at 608 runs into them and is cut off at the 32 bytes its segment still has, the
    one at 648 is gone with its frame, and the one at 688, whose D6 is now the 16th byte of the second segment, is found as before; nothing
    is joined across the gap"""
    fr = np.delete(clip_records, 20)
    got = pdt.host_tip_dcs(fr)
    assert dc.same_as_model(got, dc.model(fr))
    a, n, sm = got
    full = clip_packets[0]
    assert (sm["segments"], sm["used"], sm["skipped"]) == (2, 46, 0)
    before = [k for k in range(25) if dc.CLIP_INDICES[k] + int(full[k]["nbytes"]) <= 640]
    after = [k for k in range(25) if dc.CLIP_INDICES[k] >= 672]
    assert before == list(range(8)) and after == list(range(10, 25)) and n == 24 and dc.CLIP_INDICES[8:10] == [608, 648]
    assert a["bytes"][:8].tobytes() == full["bytes"][before].tobytes() and a["bytes"][9:].tobytes() == full["bytes"][after].tobytes()
    assert int(full[8]["nbytes"]) > 32 and (int(a[8]["stream_index"]), int(a[8]["nbytes"]), int(a[8]["complete"]), int(a[8]["doppler_raw"])) == (608, 32, 0, 0)
    assert bytes(a[8]["bytes"][:32]) == bytes(full[8]["bytes"][:32]) and not a[8]["bytes"][32:].any() and int(a[8]["id"]) == int(full[8]["id"])
    assert sm["complete"] == 22 and sm["packets"] == 24
    assert a["stream_index"][9:].tolist() == [dc.CLIP_INDICES[k] - 32 for k in after] and a["frame"][9:].tolist() == [int(full[k]["frame"]) - 1 for k in after]
    # a packet that crosses the gap is cut: drop frame 1 instead, whose slots hold the end of the packet at 12
    fr = np.delete(clip_records, 1)
    a, n, sm = pdt.host_tip_dcs(fr)
    assert dc.same_as_model((a, n, sm), dc.model(fr))
    assert (int(a[0]["stream_index"]), int(a[0]["nbytes"]), int(a[0]["complete"]), int(a[0]["doppler_ok"]), int(a[0]["id"])) == (12, 20, 0, 0, 0x9FAD2098)
    assert sm["segments"] == 2 and sm["complete"] == n - 2


@pytest.fixture(scope="module")
def kind4(pdt):
    p = pdt.synth_params(4, 50000, 1000.0, 7)
    return p, dc.kind4_records(pdt, p, 40)


def test_kind_4_frames(pdt, kind4):
    p, fr = kind4
    assert zlib.crc32(fr["bytes"][:10].tobytes()) == 0x6CCCD65A
    p3 = pdt.synth_params(3, 50000, 1000.0, 7)
    assert (p.mod_index, p.noise_gain, p.amplitude) == (p3.mod_index, p3.noise_gain, p3.amplitude)
    other = [b for b in range(103) if b not in dc.SLOTS and b not in (2, 4, 5)]
    for k in (0, 1, 39, 255, 256, 319, 320, 700):
        a, b = pdt.synth_poes_frame(p3, k), pdt.synth_poes_frame(p, k)
        assert bytes(a[other]) == bytes(b[other]) and b[2] == 8 and ((int(b[4]) & 1) << 8 | int(b[5])) == k % 320 and (a[4] ^ b[4]) & 0xFE == 0
        assert (a[103] ^ b[103]) & 0xC1 == 0
        for g in range(5):                                                          # the five parity groups over the bytes as sent
            ones = sum(bin(int(v)).count("1") for v in b[2 + 17 * g:19 + 17 * g]) + (int(b[103]) >> (5 - g) & 1)
            assert ones % 2 == 0
    # the capture carries those frames: bit j of frame 3 at 50 ksps decides the phase step's sign, as kind 3's does
    x3, x4 = pdt.synth_capture(3, 50000, 0.05, seed=7), pdt.synth_capture(4, 50000, 0.05, seed=7)
    assert x3.shape == x4.shape and (x3 != x4).any()


def test_kind_4_round_trip(pdt, kind4):
    p, fr = kind4
    got = pdt.host_tip_dcs(fr)
    assert dc.same_as_model(got, dc.model(fr))
    a, n, sm = got
    # two packets per slot group of 64 stream bytes, all complete, all with even parity, one segment
    assert (n, sm["used"], sm["skipped"], sm["segments"], sm["stream_bytes"], sm["packets"], sm["complete"], sm["doppler_bad"]) == (40, 40, 0, 1, 1280, 40, 40, 0)
    assert sm["heads"] == 40 + sm["shadowed"]
    for s in range(20):
        ta, tb = pdt.synth_dcs_packet(p, s, 0), pdt.synth_dcs_packet(p, s, 1)
        assert len(ta) == 12 + 4 * (1 + (s + 7) % 8) and len(tb) == 12 + 4 * (1 + ((s >> 3) & 1))
        for which, truth, at in ((0, ta, 64 * s), (1, tb, 64 * s + len(ta))):
            r = a[2 * s + which]
            assert int(r["stream_index"]) == at and int(r["nbytes"]) == len(truth) and bytes(r["bytes"][:len(truth)]) == bytes(truth)
            assert int(r["channel"]) == (s + 3 * which) % 8 and int(r["time_code"]) == 2 * s + which and int(r["blocks"]) == (len(truth) - 12) // 4
            assert int(r["id"]) == int.from_bytes(bytes(truth[6:10]), "big") and 0xD6 not in bytes(truth[6:len(truth) - 3])
            assert (int(r["frame"]), int(r["slot"])) == (at // 32, at % 32) and r["doppler_ok"] == 1
        assert not fr["bytes"][2 * s:2 * s + 2][:, dc.SLOTS].reshape(-1)[len(ta) + len(tb):].any()        # the rest of the group is zeros


def test_text(pdt, hand, clip_packets, tmp_path):
    some = np.concatenate([clip_packets[0]] + [pdt.host_tip_dcs(c["frames"], c["channel_max"])[0] for c in hand])
    text = pdt.format_dcs_packets(some)
    assert text == dc.format_py(some) and len(text.split(b"\n")) == len(some) + 1
    assert text.startswith(b"0.33009 7 4 1510879 9FAD2098 881.06250 D6 07 6D 97 0D DF 9F AD 20 98 ")
    assert b" - D6 " in text and b" *" in text
    path = str(tmp_path / "dcs.txt")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o644)
    assert pdt.write_dcs_packets(some, fd) == len(text)
    os.close(fd)
    assert open(path, "rb").read() == text and pdt.format_dcs_packets(some[:0]) == b""


def test_arguments(pdt, hand):
    L = pdt.lib()
    fr = by_name(hand, "shadowed")["frames"]
    out, count, sm = np.zeros(8, pdt.DCS_PACKET_DTYPE), C.c_int(-1), pdt.DcsSummary()
    ok = lambda cfg=None, frames=fr.ctypes.data, n=len(fr), o=out.ctypes.data, cap=8, c=C.byref(count), s=C.byref(sm): L.pdt_host_tip_dcs(frames, n, cfg, o, cap, c, s)
    assert ok() == 0 and count.value == 2
    assert ok(frames=None) == -1 and ok(n=1 << 31) == -1 and ok(c=None) == -1 and ok(s=None) == -1 and ok(o=None) == -1 and ok(cap=-1) == -1
    assert ok(C.byref(pdt.DcsCfg(17, 0))) == -1 and ok(C.byref(pdt.DcsCfg(16, 0))) == 0 and ok(C.byref(pdt.DcsCfg(0, 0))) == 0
    assert ok(frames=None, n=0) == 0 and count.value == 0
    assert ok(o=None, cap=0) == 0 and count.value == 2 and sm.packets == 2                     # counting only
    # the entries that need a context refuse a missing one before they touch a device
    assert L.pdt_tip_dcs(None, None, out.ctypes.data, 8, C.byref(count), C.byref(sm)) == -1
    assert L.pdt_tip_dcs_records(None, fr.ctypes.data, len(fr), None, out.ctypes.data, 8, C.byref(count), C.byref(sm)) == -1
    assert L.pdt_tip_dcs_tile() == 2048


def test_rule_under_the_sanitizers(pdt, hand, kind4, tmp_path):
    """tests/tip_dcs_host_main.cc runs the rule's host statement on exact-size heap copies of the records, the stream and the packets"""
    exe, data = str(tmp_path / "tip_dcs_host"), str(tmp_path / "cases.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "tip_dcs_host_main.cc")], check=True)
    cases = hand + dc.seam_cases(pdt, pdt.tip_dcs_tile())[:4] + [dict(frames=kind4[1], channel_max=0), dict(frames=dc.golden_records(pdt), channel_max=9)]
    with open(data, "wb") as f:
        for c in cases:
            want = len(dc.model(c["frames"], c["channel_max"])[0])
            f.write(np.array([c["channel_max"], len(c["frames"]), want], dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(c["frames"]).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"tip dcs host: ok, {len(cases)} cases" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr
