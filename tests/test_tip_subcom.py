"""The subcommutated bytes of TIP minor frames without a GPU: pdt_host_tip_subcom against a Python statement of the rule
written from the header's text (tests/tip_subcom_cases.py), field by field and the time bit for bit -- on the hand-made cases, on the
cases that put samples on tile seams and on the real recording, whose SEM and housekeeping values are written out here; the built-in
tables against POES.m's lists written out a second time; the samples' text against Python's %; every argument error; and the rule's host statement under
AddressSanitizer and UBSan in a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tip_dcs_cases as dc
import tip_subcom_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hand(pdt):
    return sc.hand_cases(pdt)


@pytest.fixture(scope="module")
def clip_records(pdt):
    return dc.golden_records(pdt)


def by_name(hand, name):
    return [c for c in hand if c["name"] == name][0]


def host(pdt, c, **kw):
    return pdt.host_tip_subcom(c["frames"], c["table"], c["trusted_only"], c["thr"], **kw)


def channel(got, c):
    a, _, off, _ = got
    return a[int(off[c]):int(off[c + 1])]


def test_built_in_tables_are_the_issues_lists(pdt):
    sem, hk = pdt.subcom_table(pdt.SUBCOM_SEM), pdt.subcom_table(pdt.SUBCOM_HK)
    assert len(sem) == 76 and int(sem["channel"].max()) + 1 == 60 and len(set(sem["channel"].tolist())) == 60 and (sem["invert"] == 1).all()
    assert len(hk) == 5 and hk["channel"].tolist() == [0, 1, 2, 3, 4] and (hk["invert"] == 0).all()
    assert sem.tobytes() == sc.listed_table(pdt, sc.sem_list(), sc.SEM_NAMES, 1).tobytes()
    assert hk.tobytes() == sc.listed_table(pdt, sc.HK_LIST, sc.HK_NAMES, 0).tobytes()
    assert [pdt.subcom_name(pdt.SUBCOM_SEM, c) for c in range(60)] == sc.SEM_NAMES and [pdt.subcom_name(pdt.SUBCOM_HK, c) for c in range(5)] == sc.HK_NAMES
    assert pdt.subcom_name(pdt.SUBCOM_SEM, 60) is None and pdt.subcom_name(pdt.SUBCOM_HK, 5) is None and pdt.subcom_name(2, 0) is None
    assert pdt.subcom_name(pdt.SUBCOM_SEM, -1) is None and len(pdt.subcom_table(2)) == 0 and len(pdt.subcom_table(-1)) == 0
    assert set(sem["byte"].tolist()) == {20, 21} and set(hk["byte"].tolist()) == {11, 14}
    t = np.zeros(3, dtype=pdt.SUBCOM_ENTRY_DTYPE)                            # a short array: the count comes back whole, three entries are written
    assert pdt.lib().pdt_subcom_table(pdt.SUBCOM_SEM, t.ctypes.data, 3) == 76 and t.tobytes() == sem[:3].tobytes()
    assert pdt.tip_subcom_tile() == 64


def test_hand_cases_cover_the_list(hand):
    assert [c["name"] for c in hand] == sc.HAND_NAMES


@pytest.mark.parametrize("k", range(len(sc.HAND_NAMES)))
def test_host_equals_the_model(pdt, hand, k):
    c = hand[k]
    got = host(pdt, c)
    assert sc.same_as_model(got, sc.model(c["frames"], c["table"], c["trusted_only"], c["thr"])), c["name"]
    sm = got[3]
    assert sm["used"] + sm["skipped"] + sm["bad_id"] == len(c["frames"]) and sm["samples"] == got[1] == int(got[2][-1])


def test_full_cycle(pdt, hand):
    """every channel's count is the sum of 320 / period over its entries: the SEM table's 36 entries of period 20, 2 of 40, 8 of 80 and 30
    of 320 give 36 * 16 + 2 * 8 + 8 * 4 + 30 = 654 samples in a full cycle of 320 frames"""
    c = by_name(hand, "sem-full-cycle")
    a, n, off, sm = host(pdt, c)
    want = [0] * 60
    for e in c["table"]:
        want[int(e["channel"])] += 320 // int(e["period"])
    assert np.diff(off).tolist() == want and n == sum(want) == 654 and sm["channels_hit"] == 60 and sm["used"] == 320
    assert (sm["byte_parity"], sm["id_parity"], sm["dropped"], sm["skipped"], sm["bad_id"]) == (0, 0, 0, 0, 0)
    assert (np.diff(a["channel"].astype(int)) >= 0).all()
    for ch in range(60):
        s = channel((a, n, off, sm), ch)
        assert (s["channel"] == ch).all() and (np.diff(s["frame"].astype(int)) > 0).all()
    a, n, off, sm = host(pdt, by_name(hand, "hk-full-cycle"))
    assert np.diff(off).tolist() == [4, 4, 4, 2, 2] and channel((a, n, off, sm), 3)["minor_id"].tolist() == [114, 274]
    assert channel((a, n, off, sm), 4)["minor_id"].tolist() == [2, 162] and channel((a, n, off, sm), 0)["minor_id"].tolist() == [48, 128, 208, 288]


def test_hand_derived_outcomes(pdt, hand):
    def run(name):
        return host(pdt, by_name(hand, name))

    a, n, off, sm = run("no-records")
    assert (len(a), n, sm) == (0, 0, dict.fromkeys(sc.SUMMARY, 0)) and len(off) == 61 and not off.any()
    a, n, off, sm = run("one-record")                                  # counter 8: 9E1 from byte 20, 9E2 from byte 21, complemented
    fr = by_name(hand, "one-record")["frames"]
    assert n == 2 and a["channel"].tolist() == [15, 16] and a["value"].tolist() == [255 - int(fr["bytes"][0, 20]), 255 - int(fr["bytes"][0, 21])]
    assert a["raw"].tolist() == [int(fr["bytes"][0, 20]), int(fr["bytes"][0, 21])] and a["flags"].tolist() == [0, 0] and a["minor_id"].tolist() == [8, 8]
    assert float(a[0]["time"]) == float(fr["time"][0]) + 20.0 * (0.1 / 104) and float(a[1]["time"]) == float(fr["time"][0]) + 21.0 * (0.1 / 104)
    a, n, off, sm = run("one-record-nothing-fires")
    assert (n, sm["used"], sm["channels_hit"]) == (0, 1, 0)
    a, n, off, sm = run("ineligible-in-the-middle")
    assert (sm["used"], sm["skipped"], sm["bad_id"]) == (57, 3, 0) and not set(a["frame"].tolist()) & {20, 21, 22}
    a, n, off, sm = run("bad-ids")
    assert (sm["used"], sm["skipped"], sm["bad_id"]) == (3, 0, 3) and sorted(set(a["frame"].tolist())) == [0, 2, 4]
    # group 0 fails in record 2: its samples carry ID_PARITY alone (byte 20 lies in group 1); trusted_only drops them.  (The bytes are noise,
    # so some samples spike: bit 8 is left out of these comparisons)
    a, n, off, sm = run("group-0-fails")
    a["flags"] &= 7
    assert (n, sm["id_parity"], sm["byte_parity"]) == (12, 2, 0) and a["flags"][a["frame"] == 2].tolist() == [2, 2] and not a["flags"][a["frame"] != 2].any()
    a, n, off, sm = run("group-0-fails-trusted")
    assert (n, sm["dropped"], sm["id_parity"], sm["byte_parity"]) == (10, 2, 0, 0) and 2 not in a["frame"].tolist()
    a, n, off, sm = run("value-group-fails")
    a["flags"] &= 7
    assert (n, sm["id_parity"], sm["byte_parity"]) == (12, 0, 2) and a["flags"][a["frame"] == 3].tolist() == [1, 1]
    assert run("value-group-fails-trusted")[3]["dropped"] == 2
    a, n, off, sm = run("both-fail")
    a["flags"] &= 7
    assert (sm["id_parity"], sm["byte_parity"]) == (2, 2) and a["flags"][a["frame"] == 1].tolist() == [3, 3]
    assert run("both-fail-trusted")[3]["dropped"] == 2
    a, n, off, sm = run("hk-byte-in-group-0")                          # byte 11 lies in group 0 itself: both bits at once
    a["flags"] &= 7
    assert a["flags"].tolist() == [0, 3, 0] and a["channel"].tolist() == [0, 0, 0]
    assert run("hk-byte-in-group-0-trusted")[0]["frame"].tolist() == [0, 2]
    # bytes 0, 1, 87 and 103 lie in no group; 2 and 86 are the first and the last that do (record 1 fails group 0, record 2 group 4)
    a, n, off, sm = run("uncovered-bytes")
    a["flags"] &= 7
    g = (a, n, off, sm)
    for ch in (0, 1, 2, 3):
        assert channel(g, ch)["flags"].tolist() == [4, 6, 4, 4]
    assert channel(g, 4)["flags"].tolist() == [0, 3, 0, 0] and channel(g, 5)["flags"].tolist() == [0, 2, 1, 0]
    fr = by_name(hand, "uncovered-bytes")["frames"]
    assert channel(g, 3)["value"].tolist() == [255 - int(v) for v in fr["bytes"][:, 103]]
    a, n, off, sm = run("uncovered-bytes-trusted")                    # an uncovered byte is trusted as far as its own parity goes, not past a failing counter
    assert sm["dropped"] == 6 + 1 and channel((a, n, off, sm), 0)["frame"].tolist() == [0, 2, 3] and channel((a, n, off, sm), 5)["frame"].tolist() == [0, 3]
    # channel 3 is fed by entries 1 and 4 in every even frame: within a frame entry 1 comes first; channel 1 and 4 are empty
    a, n, off, sm = run("own-table")
    g = (a, n, off, sm)
    s = channel(g, 3)
    assert s["entry"].tolist() == [1, 4] * 20 and s["frame"].tolist() == [f for f in range(0, 40, 2) for _ in (0, 1)] and len(channel(g, 1)) == len(channel(g, 4)) == 0
    fr = by_name(hand, "own-table")["frames"]
    assert s["value"][:2].tolist() == [(int(fr["bytes"][0, 31]) & 0x7E) >> 1, int(fr["bytes"][0, 30])] and sm["channels_hit"] == 4
    assert channel(g, 0)["entry"].tolist() == [2] * 27 + [2, 5] + [2] * 12          # counter 7 is frame 27: entry 2 comes before entry 5 there
    assert channel(g, 5)["minor_id"].tolist() == [i for i in [(300 + k) % 320 for k in range(40)] if i % 4 == 3]


def test_spikes(pdt, hand):
    def flags(name):
        return host(pdt, by_name(hand, name))[0]["flags"].tolist()

    assert flags("spike") == [0, 0, 8, 0, 0, 0, 8, 0, 0, 0]
    # 140 and 60 side by side: the reference zeroes the first and then tests 60 against 0; here both are flagged and keep their values
    a = host(pdt, by_name(hand, "spike-beside-spike"))
    assert a[0]["flags"].tolist() == [0, 0, 8, 8, 0, 0, 0, 0, 0, 0] and a[0]["value"][2:4].tolist() == [140, 60] and a[3]["spikes"] == 2
    assert flags("first-and-last") == [0] * 10
    # the samples 1, 4, 7 and 10 stand 20, 21, 255 and 254 above their neighbours: "greater than", so 20 is no spike under 20
    assert flags("threshold-0") == flags("threshold-20") == [0, 0, 0, 0, 8, 0, 0, 8, 0, 0, 8, 0]
    assert flags("threshold-21") == [0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 8, 0] and flags("threshold-254") == [0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0]
    assert flags("threshold-255") == [0] * 12
    a = host(pdt, by_name(hand, "spike-on-decoded-values"))[0]           # the values: 0 0 15 0 1 1 1 1 1 1 -- the raw bytes differ far more
    assert a["value"].tolist() == [0, 0, 15, 0, 1, 1, 1, 1, 1, 1] and a["flags"].tolist() == [0, 0, 8, 0, 0, 0, 0, 0, 0, 0]


def test_cap_smaller_than_the_count(pdt, hand):
    c = by_name(hand, "own-table")
    full = host(pdt, c)
    mid = int(full[2][3]) + 5                                          # inside channel 3
    for cap in (0, 1, mid, full[1], full[1] + 3):
        a, n, off, sm = host(pdt, c, cap=cap)
        assert n == full[1] and sm == full[3] and off.tobytes() == full[2].tobytes() and len(a) == min(cap, n) and a.tobytes() == full[0][:cap].tobytes()
    # a spike in the last sample that fits keeps its flag although its right neighbour is not written, and nothing behind cap is
    c = by_name(hand, "spike")
    a, n, off, sm = host(pdt, c, cap=3)
    assert a["flags"].tolist() == [0, 0, 8] and sm["spikes"] == 2
    out, count, s = np.full(4 * 24, 0x55, dtype=np.uint8).view(pdt.SUBCOM_SAMPLE_DTYPE), C.c_int(0), pdt.SubcomSummary()
    fr, t = c["frames"], c["table"]
    assert pdt.lib().pdt_host_tip_subcom(fr.ctypes.data, len(fr), t.ctypes.data, len(t), None, out.ctypes.data, 3, C.byref(count), None, C.byref(s)) == 0
    assert count.value == 10 and out[:3].tobytes() == a.tobytes() and out[3].tobytes() == b"\x55" * 24


@pytest.mark.parametrize("k", range(len(sc.SEAM_NAMES)))
def test_seam_cases_on_the_host(pdt, k):
    c = sc.seam_cases(pdt, pdt.tip_subcom_tile())[k]
    assert c["name"] == sc.SEAM_NAMES[k]
    assert sc.same_as_model(host(pdt, c), sc.model(c["frames"], c["table"], c["trusted_only"], c["thr"])), c["name"]


def test_real_recording_sem(pdt, clip_records):
    got = pdt.host_tip_subcom(clip_records, pdt.SUBCOM_SEM)
    assert sc.same_as_model(got, sc.model(clip_records, pdt.subcom_table(pdt.SUBCOM_SEM)))
    a, n, off, sm = got
    ids = [(int(b[4]) & 1) << 8 | int(b[5]) for b in clip_records["bytes"]]
    assert ids == list(range(275, 320)) + [0, 1]
    assert n == 95 and sm == dict(used=47, skipped=0, bad_id=0, samples=95, dropped=0, byte_parity=0, id_parity=0, spikes=0, channels_hit=44)
    value = lambda name: channel(got, sc.SEM_NAMES.index(name))["value"].tolist()
    assert value("9E1") == [71, 73] and value("9E2") == [31, 34] and value("3EM") == [13, 13, 13] and value("0EFH") == [0, 0, 34]
    assert not a["flags"].any()
    # trusted_only has nothing to drop, and the samples are the same
    assert sc.same(pdt.host_tip_subcom(clip_records, pdt.SUBCOM_SEM, trusted_only=True), got)


def test_real_recording_housekeeping(pdt, clip_records):
    got = pdt.host_tip_subcom(clip_records, pdt.SUBCOM_HK)
    assert sc.same_as_model(got, sc.model(clip_records, pdt.subcom_table(pdt.SUBCOM_HK)))
    a, n, off, sm = got
    assert n == 3 and a["channel"].tolist() == [0, 1, 2] and a["value"].tolist() == [0, 174, 175] and a["minor_id"].tolist() == [288, 290, 280]
    # counter 288 is the frame at 1.58163 s; the sample's time is its byte's own, 11 bytes into the frame
    f = int(a[0]["frame"])
    assert "%.5f" % float(clip_records["time"][f]) == "1.58163" and float(a[0]["time"]) == float(clip_records["time"][f]) + 11.0 * (0.1 / 104)
    assert off.tolist() == [0, 1, 2, 3, 3, 3] and not a["flags"].any()
    assert pdt.format_subcom(a, pdt.SUBCOM_HK).split(b"\n")[0] == b"1.59221 STX1 288 0 -"


def test_text(pdt, hand, clip_records, tmp_path):
    sem = pdt.host_tip_subcom(clip_records, pdt.SUBCOM_SEM)[0]
    assert pdt.format_subcom(sem, pdt.SUBCOM_SEM) == sc.format_py(sem, sc.SEM_NAMES)
    some = np.concatenate([host(pdt, c)[0] for c in hand])
    text = pdt.format_subcom(some)
    assert text == sc.format_py(some) and len(text.split(b"\n")) == len(some) + 1
    letters = {line.split()[-1] for line in text.decode().split("\n") if line}
    assert {"-", "b", "i", "bi", "u", "iu", "s"} <= letters and all(v == "-" or v == "".join(ch for ch in "bius" if ch in v) for v in letters)
    # a channel the named table does not have is written as c<channel>
    assert pdt.format_subcom(some, pdt.SUBCOM_HK) == sc.format_py(some, sc.HK_NAMES) and b" c15 " in pdt.format_subcom(some, pdt.SUBCOM_HK)
    path = str(tmp_path / "sem.txt")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o644)
    assert pdt.write_subcom(sem, fd, pdt.SUBCOM_SEM) == len(sc.format_py(sem, sc.SEM_NAMES))
    os.close(fd)
    assert open(path, "rb").read() == sc.format_py(sem, sc.SEM_NAMES) and pdt.format_subcom(sem[:0]) == b""


def test_arguments(pdt, hand):
    L = pdt.lib()
    c = by_name(hand, "own-table")
    fr, tab = c["frames"], c["table"]
    out, count, sm, off = np.zeros(256, pdt.SUBCOM_SAMPLE_DTYPE), C.c_int(-1), pdt.SubcomSummary(), np.zeros(129, np.uint64)

    def call(frames=fr.ctypes.data, n=len(fr), t=tab, nt=None, cfg=None, o=out.ctypes.data, cap=256, cn=C.byref(count), of=off.ctypes.data, s=C.byref(sm)):
        return L.pdt_host_tip_subcom(frames, n, t.ctypes.data if t is not None else None, len(t) if nt is None else nt, cfg, o, cap, cn, of, s)

    full = host(pdt, c)
    assert call() == 0 and count.value == full[1]
    assert call(frames=None) == -1 and call(n=1 << 31) == -1 and call(cn=None) == -1 and call(s=None) == -1 and call(o=None) == -1 and call(cap=-1) == -1
    assert call(t=None, nt=3) == -1 and call(nt=0) == -1
    assert call(of=None) == 0                                            # the offsets are optional
    assert call(frames=None, n=0) == 0 and count.value == 0
    assert call(o=None, cap=0) == 0 and count.value == full[1] and sm.samples == full[1] and off[:7].tobytes() == full[2].tobytes()      # counting only
    # thresholds: 0 .. 255 are allowed
    cfg = lambda tr, th: C.byref(pdt.SubcomCfg(tr, th))
    assert call(cfg=cfg(0, 256)) == -1 and call(cfg=cfg(0, 255)) == 0 and call(cfg=cfg(1, 0)) == 0 and call(cfg=cfg(7, 1)) == 0
    # every way a table entry can be wrong; and the limits that are allowed
    good = (3, 103, 320, 319, 1, 7, 1)
    assert call(t=sc.table(pdt, [good])) == 0
    for k, v in ((0, 128), (1, 104), (2, 0), (2, 3), (2, 640), (2, 321), (3, 320), (4, 0), (5, 8), (6, 2)):
        e = list(good)
        e[k] = v
        assert call(t=sc.table(pdt, [(0, 0, 1, 0, 255, 0, 0), tuple(e)])) == -1, (k, v)
    assert call(t=sc.table(pdt, [(0, 0, 20, 20, 255, 0, 0)])) == -1
    many = sc.table(pdt, [(k % 128, k % 104, 320, k, 255, 0, 0) for k in range(257)])
    assert call(t=many) == -1 and call(t=many[:256]) == 0
    # more samples than an int counts: 2^31 - 1 records are refused for their number alone, 2^30 for what a table that fires three entries in a frame could give
    three = sc.table(pdt, [(0, 0, 1, 0, 255, 0, 0)] * 3)
    assert call(n=1 << 30, t=three) == -1
    # the entries that need a context refuse a missing one before they touch a device
    assert L.pdt_tip_subcom(None, tab.ctypes.data, len(tab), None, out.ctypes.data, 8, C.byref(count), None, C.byref(sm)) == -1
    assert L.pdt_tip_subcom_records(None, fr.ctypes.data, len(fr), tab.ctypes.data, len(tab), None, out.ctypes.data, 8, C.byref(count), None, C.byref(sm)) == -1


def test_rule_under_the_sanitizers(pdt, hand, clip_records, tmp_path):
    """tests/tip_subcom_host_main.cc runs the rule's host statement on exact-size heap copies of the records, the table, the offsets, the
    values and the samples"""
    exe, data = str(tmp_path / "tip_subcom_host"), str(tmp_path / "cases.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "tip_subcom_host_main.cc")], check=True)
    cases = hand + sc.seam_cases(pdt, pdt.tip_subcom_tile()) + [dict(frames=sc.kind4_records(pdt, 400, flips=60), table=sc.big_table(pdt), trusted_only=False, thr=0)]
    with open(data, "wb") as f:
        for c in cases:
            want = sc.model(c["frames"], c["table"], c["trusted_only"], c["thr"])[2]
            f.write(np.array([len(c["frames"]), len(c["table"]), int(c["trusted_only"]), c["thr"], want["samples"], want["spikes"]], dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(c["table"]).tobytes())
            f.write(np.ascontiguousarray(c["frames"]).tobytes())
        for which in (0, 1):                                             # the built-in tables, from the header itself (a table of 0 entries asks for them)
            want = sc.model(clip_records, pdt.subcom_table(which))[2]
            f.write(np.array([len(clip_records), 0, which, 0, want["samples"], want["spikes"]], dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(clip_records).tobytes())
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"tip subcom host: ok, {len(cases) + 2} cases" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr
