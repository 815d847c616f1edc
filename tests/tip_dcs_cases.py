"""Cases for the DCS decommutation of TIP minor frames, shared by tests/test_tip_dcs.py (host) and tests/test_gpu_tip_dcs.py
(kernels): a Python statement of the rule written from the text of include/pdt.h -- not from the C --, builders for packets, streams and
records, the hand-made streams, the streams that put packets on tile seams, and the real recording's frames as records."""
import os

import numpy as np

SLOTS = [18, 19, 24, 25, 28, 29, 32, 33, 40, 41, 44, 45, 52, 53, 56, 57, 60, 61, 64, 65, 68, 69, 72, 73, 76, 77, 86, 87, 90, 91, 94, 95]
VALID_CODES = [0x0, 0x3, 0x5, 0x6, 0x9, 0xA, 0xC, 0xF]
INVALID_CODES = [c for c in range(16) if c not in VALID_CODES]
SUMMARY = ("used", "skipped", "segments", "stream_bytes", "heads", "shadowed", "bad_code", "packets", "complete", "doppler_bad")
FIELDS = ("time", "stream_index", "frame", "time_code", "id", "doppler_raw", "slot", "channel", "blocks", "nbytes", "complete", "doppler_ok", "pad", "bytes")


def code_valid(c):
    n1 = c >> 1
    return (c & 1) == (((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1)


assert [c for c in range(16) if code_valid(c)] == VALID_CODES


def model(frames, channel_max=0):
    """the rule, straight from its text: (list of packet dicts, summary dict)"""
    cm = 8 if channel_max == 0 else channel_max
    n = len(frames)
    ok = [int(f["complete"]) == 1 and int(f["nbytes"]) == 104 for f in frames]
    sm = dict.fromkeys(SUMMARY, 0)
    packets, i, counted = [], 0, 0
    while i < n:
        if not ok[i]:
            sm["skipped"] += 1
            i += 1
            continue
        j = i + 1
        while j < n and ok[j] and int(frames[j]["bit_index"]) - int(frames[j - 1]["bit_index"]) == 832:
            j += 1
        S = [int(frames[r]["bytes"][b]) for r in range(i, j) for b in SLOTS]
        sm["segments"] += 1
        sm["used"] += j - i
        sm["stream_bytes"] += len(S)
        end = 0
        for k in range(len(S) - 2):
            if S[k] != 0xD6 or S[k + 1] >= cm:
                continue
            c = S[k + 2] >> 4
            if not code_valid(c):
                sm["bad_code"] += 1
                continue
            sm["heads"] += 1
            if k < end:
                sm["shadowed"] += 1
                continue
            blocks = (c >> 1) + 1
            L = 12 + 4 * blocks
            end = k + L
            nb = min(L, len(S) - k)
            r, slot = i + k // 32, k % 32
            p = dict(time=float(frames[r]["time"]) + float(SLOTS[slot]) * (0.1 / 104), stream_index=counted * 32 + k, frame=r, slot=slot, channel=S[k + 1],
                     blocks=blocks, nbytes=nb, complete=int(nb == L), bytes=bytes(S[k:k + nb]) + bytes(44 - nb), pad=bytes(2),
                     time_code=((S[k + 3] & 31) << 16 | S[k + 4] << 8 | S[k + 5]) if nb >= 6 else 0,
                     id=int.from_bytes(bytes(S[k + 6:k + 10]), "big") if nb >= 10 else 0, doppler_ok=0, doppler_raw=0)
            if nb == L:
                w = S[k + L - 3] << 16 | S[k + L - 2] << 8 | S[k + L - 1]
                p["doppler_ok"] = int(bin(w).count("1") % 2 == 0)
                p["doppler_raw"] = (w >> 1) - (1 << 22)
                sm["complete"] += 1
                sm["doppler_bad"] += 1 - p["doppler_ok"]
            packets.append(p)
            sm["packets"] += 1
        counted += j - i
        i = j
    return packets, sm


def as_dicts(arr):
    return [{k: (bytes(r[k]) if k in ("bytes", "pad") else float(r[k]) if k == "time" else int(r[k])) for k in FIELDS} for r in arr]


def same_as_model(got, want, cap=None):
    """(packets array, count, summary) against the model's (packets, summary), field by field; the time bit for bit"""
    arr, count, sm = got
    packets, wsm = want
    keep = len(packets) if cap is None else min(cap, len(packets))
    if count != len(packets) or sm != wsm or len(arr) != keep:
        return False
    for a, b in zip(as_dicts(arr), packets[:keep]):
        for k in FIELDS:
            if k == "time":
                if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes():
                    return False
            elif a[k] != b[k]:
                return False
    return True


def same(a, b):
    """two (packets array, count, summary) results, byte for byte"""
    return a[1] == b[1] and a[2] == b[2] and len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes()


def packet(channel, blocks, time_code, ident, salt=0, flip=False, doppler=None):
    """a packet as a platform's message is relayed: D6, channel, length code, time code, ID, data (no D6 among them), Doppler word with its
    even parity (flip: one bit of the word complemented)"""
    n1 = blocks - 1
    code = (n1 << 1) | (((n1 >> 2) ^ (n1 >> 1) ^ n1) & 1)
    L = 12 + 4 * blocks
    rng = np.random.default_rng(1000 + 64 * salt + blocks)
    data = [int(v) for v in rng.integers(0, 256, L - 13)]
    data = [0xD7 if v == 0xD6 else v for v in data]
    v = int(rng.integers(0, 1 << 23)) if doppler is None else doppler
    w = (v << 1) | (bin(v).count("1") & 1)
    if flip:
        w ^= 1 << 9
    b = [0xD6, channel, (code << 4) | (salt & 15), (time_code >> 16) & 31, (time_code >> 8) & 255, time_code & 255] + list(ident.to_bytes(4, "big")) + data
    b += [(w >> 16) & 255, (w >> 8) & 255, w & 255]
    assert len(b) == L
    return bytes(b)


def records(pdt, stream, bit0=18, t0=0.3125, salt=7):
    """stream (a multiple of 32 bytes) as consecutive complete records 832 bits apart; every other byte of a frame is noise that holds D6
    pairs too (the decommutation reads the 32 slots only)"""
    assert len(stream) % 32 == 0
    n = len(stream) // 32
    fr = np.zeros(n, dtype=pdt.FRAME_DTYPE)
    rng = np.random.default_rng(salt)
    body = rng.integers(0, 256, (n, 104)).astype(np.uint8)
    body[:, 0], body[:, 1], body[:, 20], body[:, 21], body[:, 22] = 0xED, 0xE2, 0xD6, 0x01, 0x30
    s = np.frombuffer(bytes(stream), dtype=np.uint8).reshape(n, 32)
    body[:, SLOTS] = s
    fr["bytes"] = body
    fr["bit_index"] = bit0 + 832 * np.arange(n)
    fr["time_src"] = 37 * np.arange(n)
    fr["time"] = t0 + np.arange(n) * 0.1 + np.arange(n) * 1e-7 / 3
    fr["nbytes"], fr["complete"] = 104, 1
    return fr


def place(length, items):
    """a stream of `length` zeros with the byte strings of items = [(position, bytes)] written over it"""
    s = bytearray(length)
    for at, b in items:
        assert 0 <= at and at + len(b) <= length
        s[at:at + len(b)] = b
    return bytes(s)


def split(fr, at, gap=832):
    """the records with a gap in the bit index in front of record `at`: a segment break"""
    out = fr.copy()
    out["bit_index"][at:] += gap
    return out


def hand_cases(pdt):
    """[dict(name, frames, channel_max)]: the issue's hand-made streams"""
    cases = []

    def add(name, frames, channel_max=0):
        cases.append(dict(name=name, frames=frames, channel_max=channel_max))

    # a D6 0x <valid> pair inside a packet's data: shadowed, the packet intact
    p = bytearray(packet(3, 4, 0x12345, 0xCAFE0123, 1))
    p[12:15] = bytes([0xD6, 0x02, 0x5A])
    add("shadowed", records(pdt, place(96, [(5, bytes(p)), (5 + 28, packet(1, 1, 77, 0x01020304, 2))])))
    # D6 as a segment's first byte
    add("first-byte", records(pdt, place(64, [(0, packet(0, 2, 5, 0xA0B0C0D0, 3))])))
    add("first-byte-second-segment", split(records(pdt, place(128, [(0, packet(0, 2, 5, 0xA0B0C0D0, 3)), (64, packet(6, 8, 6, 0xFFFFFFFF, 4))])), 2))
    # D6 in a segment's last and second-to-last byte: what would follow lies behind a gap
    add("last-byte", split(records(pdt, place(128, [(63, packet(2, 1, 9, 0x11223344, 5))])), 2))
    add("second-to-last-byte", split(records(pdt, place(128, [(62, packet(2, 1, 9, 0x11223344, 5))])), 2))
    add("third-to-last-byte", split(records(pdt, place(128, [(61, packet(2, 1, 9, 0x11223344, 5))])), 2))
    add("stream-ends", records(pdt, place(64, [(20, packet(4, 8, 1, 2, 6)), (63, b"\xD6")])))
    # channel byte 7, 8 and 9 under channel_max 8 and 9 (and 16, and 1)
    chan = place(128, [(0, packet(7, 1, 1, 0x70, 7)), (16, packet(8, 1, 2, 0x80, 8)), (32, packet(9, 1, 3, 0x90, 9)), (48, packet(0, 1, 4, 0x00, 10)),
                       (64, packet(15, 1, 5, 0xF0, 11)), (80, packet(16, 1, 6, 0x100, 12))])
    for cm in (0, 8, 9, 16, 1):
        add(f"channels-{cm}", records(pdt, chan), cm)
    # each of the eight invalid length nibbles
    add("bad-codes", records(pdt, place(96, [(4 + 8 * k, bytes([0xD6, k % 8, (c << 4) | 5])) for k, c in enumerate(INVALID_CODES)] + [(70, packet(5, 2, 8, 9, 13))])))
    # a flipped Doppler bit
    add("doppler-flipped", records(pdt, place(64, [(3, packet(1, 3, 10, 11, 14, flip=True)), (3 + 24, packet(1, 3, 12, 13, 15))])))
    # incomplete and nbytes != 104 records between segments
    fr = records(pdt, place(256, [(10, packet(0, 8, 1, 1, 16)), (60, packet(1, 8, 2, 2, 17)), (120, packet(2, 8, 3, 3, 18)), (170, packet(3, 8, 4, 4, 19)),
                                  (226, packet(4, 4, 5, 5, 20))]))
    fr["complete"][2] = 0
    fr["nbytes"][5] = 103
    fr["complete"][6] = 2
    add("ineligible-between", fr)
    # records out of order: every record a segment of its own
    fr = records(pdt, place(128, [(2, packet(0, 1, 1, 1, 21)), (40, packet(1, 1, 2, 2, 22)), (60, packet(2, 2, 3, 3, 23)), (100, packet(3, 1, 4, 4, 24))]))
    add("out-of-order", fr[::-1].copy())
    add("no-records", records(pdt, b""))
    # the longest and the shortest packets back to back, the last one cut off by the end
    add("back-to-back", records(pdt, place(128, [(0, packet(0, 8, 1, 1, 25)), (44, packet(1, 1, 2, 2, 26)), (60, packet(2, 8, 3, 3, 27)), (104, packet(3, 8, 4, 4, 28)[:24])])))
    return cases


HAND_NAMES = ["shadowed", "first-byte", "first-byte-second-segment", "last-byte", "second-to-last-byte", "third-to-last-byte", "stream-ends",
              "channels-0", "channels-8", "channels-9", "channels-16", "channels-1", "bad-codes", "doppler-flipped", "ineligible-between",
              "out-of-order", "no-records", "back-to-back"]


def seam_cases(pdt, T):
    """[dict(name, frames, channel_max)]: 3 T bytes of stream with packets, shadowed heads and segment breaks on the seams of tiles of T bytes"""
    assert T % 32 == 0 and T >= 128
    cases = []
    fill = [(40 + 52 * k, packet(k % 8, 1 + k % 8, k, 0x1000 + k, 30 + k % 16)) for k in range((T - 200) // 52)]       # packets all over the first tile

    def add(name, items, breaks=(), skip=()):
        fr = records(pdt, place(3 * T, fill + items))
        for b in breaks:
            fr = split(fr, b)
        for r in skip:
            fr["complete"][r] = 0
        cases.append(dict(name=name, frames=fr, channel_max=0))

    for d in (-2, -1, 0, 1):
        add(f"head-at-seam{d:+d}", [(T + d, packet(1, 8, 100 + d, 0xABCD0000, 3)), (2 * T + d, packet(2, 1, 200 + d, 0xABCD0001, 4))])
    add("one-byte-across", [(T - 43, packet(1, 8, 1, 1, 5)), (2 * T - 15, packet(2, 1, 2, 2, 6))])
    add("43-bytes-across", [(T - 1, packet(1, 8, 1, 1, 5)), (T + 43, packet(3, 2, 3, 3, 7)), (2 * T - 1, packet(2, 8, 2, 2, 6))])
    p = bytearray(packet(1, 8, 1, 1, 8))
    p[10:13] = bytes([0xD6, 0x00, 0x00])
    add("shadowed-head-first-in-tile", [(T - 10, bytes(p)), (T + 34, packet(4, 1, 9, 9, 9))])
    add("shadowed-head-opens-nothing", [(T - 10, bytes(p)), (T + 20, packet(4, 1, 9, 9, 9)), (T + 36, packet(5, 1, 9, 9, 9))])
    # a segment break on the seam: a D6 one byte in front of it is no head, the packet that crosses it is cut, the one behind it is found
    for d in (-1, 0, 1):
        add(f"break-on-seam-head{d:+d}", [(T + d, packet(1, 8, 1, 1, 10)), (T - 60, packet(2, 8, 2, 2, 11)), (2 * T - 20, packet(3, 8, 3, 3, 12))],
            breaks=(T // 32, 2 * T // 32))
    add("break-one-record-off-seam", [(T - 40, packet(1, 8, 1, 1, 10)), (T + 30, packet(2, 8, 2, 2, 11)), (2 * T - 3, packet(3, 8, 3, 3, 12))],
        breaks=(T // 32 - 1, T // 32 + 1, 2 * T // 32))
    # an ineligible record in front: stream indices and the tiles' seams part ways
    add("skipped-record-shifts-the-stream", [(T + 31, packet(1, 8, 1, 1, 13)), (T + 32 + 43, packet(2, 8, 2, 2, 14)), (2 * T + 20, packet(3, 8, 3, 3, 15))], skip=(3,))
    add("every-record-its-own-segment", [(T - 20, packet(1, 1, 1, 1, 13)), (T, packet(2, 1, 2, 2, 14)), (T + 16, packet(2, 1, 2, 2, 14)), (T + 29, packet(2, 1, 2, 2, 14))],
        breaks=tuple(range(T // 32 - 2, T // 32 + 3)))
    return cases


def kind4_records(pdt, p, nframes, first=0):
    """the frames first .. first + nframes - 1 a kind 4 capture carries, as records"""
    fr = np.zeros(nframes, dtype=pdt.FRAME_DTYPE)
    for k in range(nframes):
        fr["bytes"][k] = pdt.synth_poes_frame(p, first + k)
    fr["bit_index"] = 18 + 832 * np.arange(nframes)
    fr["time"] = 0.0125 + np.arange(nframes) * 0.1
    fr["nbytes"], fr["complete"] = 104, 1
    return fr


def golden_records(pdt, name="clip.c10000.txt"):
    """the frames of a committed minor-frame text as records 832 bits apart (the text keeps time and bytes, not the bit index)"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    rows = [line.split() for line in open(os.path.join(golden, name)).read().split("\n")]
    rows = [r for r in rows if len(r) == 105]
    fr = np.zeros(len(rows), dtype=pdt.FRAME_DTYPE)
    for k, r in enumerate(rows):
        fr["time"][k] = float(r[0].rstrip("i"))
        fr["inverted"][k] = r[0].endswith("i")
        fr["bytes"][k] = [int(h, 16) for h in r[1:]]
    fr["bit_index"] = 1000 + 832 * np.arange(len(rows))
    fr["nbytes"], fr["complete"] = 104, 1
    return fr


CLIP_INDICES = [12, 64, 173, 213, 245, 265, 328, 396, 608, 648, 688, 728, 772, 906, 1034, 1069, 1109, 1125, 1165, 1189, 1232, 1252, 1402, 1471, 1495]


def format_py(packets):
    """the packets' text with Python's %"""
    out = b""
    for r in packets:
        d = "-" if not r["complete"] else ("" if r["doppler_ok"] else "*") + "%.5f" % (int(r["doppler_raw"]) / 32.0)
        line = "%.5f %u %u %07u %08X %s " % (float(r["time"]), int(r["channel"]), int(r["blocks"]), int(r["time_code"]), int(r["id"]), d)
        line += "".join("%02X " % int(v) for v in r["bytes"][:int(r["nbytes"])]) + "\n"
        out += line.encode()
    return out
