"""Cases for the decommutation of TIP minor frames' subcommutated bytes, shared by tests/test_tip_subcom.py (host) and
tests/test_gpu_tip_subcom.py (kernels): a Python statement of the rule written from the text of include/pdt.h -- not from the C --, the
built-in tables written out once more from POES.m's lists (as include/pdt.h names them), builders for records and tables, the hand-made cases, the cases that put samples on
tile seams, and the large ones."""
import numpy as np

SUMMARY = ("used", "skipped", "bad_id", "samples", "dropped", "byte_parity", "id_parity", "spikes", "channels_hit")
FIELDS = ("time", "frame", "minor_id", "channel", "entry", "value", "raw", "flags", "pad")
BYTE_PARITY, ID_PARITY, UNCOVERED, SPIKE = 1, 2, 4, 8
DIVISORS = [d for d in range(1, 321) if 320 % d == 0]

A, B = 20, 21
SEM_NAMES = ("0P1 0P2 0P3 0P4 0P5 0P6 0E1 0E2 0E3 9P1 9P2 9P3 9P4 9P5 9P6 9E1 9E2 9E3 P6 P7 P8 P9 "
             "0EFL 3EFL 0PFL 3PFL 0EFH 3EFH 0PFH 3PFH 0EM 0PM 0DEM 0DPM 3EM 3PM 3DEM 3DPM 0DE1 0DE2 3DE1 3DE2 "
             "0DP1 0DP2 3DP1 3DP2 0EBKL 0EBKH 3PBKL 0DE3 0DE4 3DE3 3DE4 0DP3 0DP4 3DP3 3DP4 0PBKL 0PBKH 3PBKH").split()
HK_NAMES = ["STX1", "STX2", "STX3", "SARR-A", "SARR-B"]


def sem_list():
    """the SEM table as POES.m:1340-1377 and 1561-1621 list it, in the header's channel order: [(name, byte, period, phase, mask, shift)], every entry inverted"""
    rows = [("0P1", B, 20, 0)]
    meped = ["0P2", "0P3", "0P4", "0P5", "0P6", "0E1", "0E2", "0E3", "9P1", "9P2", "9P3", "9P4", "9P5", "9P6", "9E1", "9E2", "9E3", "P6"]
    for p in range(1, 10):
        rows += [(meped[2 * p - 2], A, 20, p), (meped[2 * p - 1], B, 20, p)]
    rows += [("P7", A, 20, 10), ("P8", B, 40, 10), ("P9", B, 40, 30)]
    for phase, a, b in ((13, "0EFL", "3EFL"), (14, "0PFL", "3PFL"), (15, "0EFH", "3EFH"), (16, "0PFH", "3PFH")):
        rows += [(a, A, 20, phase), (b, B, 20, phase)]
    rows += [("0EM", A, 20, 17, 0xF0, 4), ("0PM", A, 20, 17, 0x0F, 0), ("0DEM", B, 20, 17)]
    rows += [("0DPM", A, 20, 18), ("3EM", B, 20, 18, 0xF0, 4), ("3PM", B, 20, 18, 0x0F, 0)]
    rows += [("3DEM", A, 20, 19), ("3DPM", B, 20, 19)]
    rows += [("0DE1", A, 80, 11), ("0DE2", B, 80, 11), ("3DE1", A, 80, 31), ("3DE2", B, 80, 31)]
    for ids, a, b in (((51, 131, 211), "0DP1", "0DP2"), ((71, 151, 231), "3DP1", "3DP2"), ((291,), "0EBKL", "0EBKH")):
        for i in ids:
            rows += [(a, A, 320, i), (b, B, 320, i)]
    rows += [("3PBKL", B, 320, 311)]
    rows += [("0DE3", A, 80, 12), ("0DE4", B, 80, 12), ("3DE3", A, 80, 32), ("3DE4", B, 80, 32)]
    for ids, a, b in (((52, 132, 212), "0DP3", "0DP4"), ((72, 152, 232), "3DP3", "3DP4"), ((292,), "0PBKL", "0PBKH")):
        for i in ids:
            rows += [(a, A, 320, i), (b, B, 320, i)]
    rows += [("3PBKH", B, 320, 312)]
    return [r + (0xFF, 0) if len(r) == 4 else r for r in rows]


HK_LIST = [("STX1", 11, 80, 48, 0xFF, 0), ("STX2", 11, 80, 50, 0xFF, 0), ("STX3", 11, 80, 40, 0xFF, 0), ("SARR-A", 14, 160, 114, 0xFF, 0),
           ("SARR-B", 14, 160, 2, 0xFF, 0)]


def table(pdt, entries):
    """[(channel, byte, period, phase, mask, shift, invert)] -> SUBCOM_ENTRY_DTYPE records"""
    t = np.zeros(len(entries), dtype=pdt.SUBCOM_ENTRY_DTYPE)
    for k, e in enumerate(entries):
        t[k] = tuple(e) + (0,)
    return t


def listed_table(pdt, rows, names, invert):
    return table(pdt, [(names.index(n), byte, period, phase, mask, shift, invert) for n, byte, period, phase, mask, shift in rows])


def group_fails(b, g):
    ones = sum(bin(int(v)).count("1") for v in b[2 + 17 * g:19 + 17 * g]) + ((int(b[103]) >> (5 - g)) & 1)
    return ones % 2 == 1


def model(frames, tab, trusted_only=False, thr=0):
    """the rule, straight from its text: (list of sample dicts in order, offsets list, summary dict)"""
    thr = 20 if thr == 0 else thr
    nchan = max(int(e["channel"]) for e in tab) + 1
    per = [[] for _ in range(nchan)]
    sm = dict.fromkeys(SUMMARY, 0)
    for i, f in enumerate(frames):
        if not (int(f["complete"]) == 1 and int(f["nbytes"]) == 104):
            sm["skipped"] += 1
            continue
        b = f["bytes"]
        ident = (int(b[4]) & 1) << 8 | int(b[5])
        if ident >= 320:
            sm["bad_id"] += 1
            continue
        sm["used"] += 1
        fails = [group_fails(b, g) for g in range(5)]
        for k, e in enumerate(tab):
            if ident % int(e["period"]) != int(e["phase"]):
                continue
            byte = int(e["byte"])
            g = (byte - 2) // 17 if 2 <= byte <= 86 else -1
            flags = (BYTE_PARITY if g >= 0 and fails[g] else 0) | (ID_PARITY if fails[0] else 0) | (UNCOVERED if g < 0 else 0)
            if trusted_only and flags & 3:
                sm["dropped"] += 1
                continue
            raw = int(b[byte])
            value = (((255 - raw) if int(e["invert"]) else raw) & int(e["mask"])) >> int(e["shift"])
            per[int(e["channel"])].append(dict(time=float(f["time"]) + float(byte) * (0.1 / 104), frame=i, minor_id=ident, channel=int(e["channel"]), entry=k,
                                               value=value, raw=raw, flags=flags, pad=bytes(5)))
    offsets = [0]
    for s in per:
        for j in range(1, len(s) - 1):
            if abs(s[j - 1]["value"] - s[j]["value"]) > thr and abs(s[j + 1]["value"] - s[j]["value"]) > thr:
                s[j]["flags"] |= SPIKE
                sm["spikes"] += 1
        offsets.append(offsets[-1] + len(s))
        sm["channels_hit"] += len(s) != 0
        sm["byte_parity"] += sum(1 for v in s if v["flags"] & BYTE_PARITY)
        sm["id_parity"] += sum(1 for v in s if v["flags"] & ID_PARITY)
    sm["samples"] = offsets[-1]
    return [v for s in per for v in s], offsets, sm


def as_dicts(arr):
    return [{k: (bytes(r[k]) if k == "pad" else float(r[k]) if k == "time" else int(r[k])) for k in FIELDS} for r in arr]


def same_as_model(got, want, cap=None):
    """(samples array, count, offsets, summary) against the model's (samples, offsets, summary), field by field; the time bit for bit"""
    arr, count, off, sm = got
    samples, woff, wsm = want
    keep = len(samples) if cap is None else min(cap, len(samples))
    if count != len(samples) or sm != wsm or len(arr) != keep or [int(v) for v in off] != woff:
        return False
    for a, b in zip(as_dicts(arr), samples[:keep]):
        for k in FIELDS:
            if k == "time":
                if np.float64(a[k]).tobytes() != np.float64(b[k]).tobytes():
                    return False
            elif a[k] != b[k]:
                return False
    return True


def same(a, b):
    """two (samples array, count, offsets, summary) results, byte for byte"""
    return a[1] == b[1] and a[3] == b[3] and a[2].tobytes() == b[2].tobytes() and len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes()


def fix_parity(fr):
    """bit 5 - g of byte 103 set so that every group g of every record passes"""
    body = fr["bytes"]
    ones = np.unpackbits(body[:, 2:87], axis=1).reshape(len(fr), 5, 136).sum(axis=2) & 1
    for g in range(5):
        body[:, 103] = (body[:, 103] & ~np.uint8(1 << (5 - g))) | (ones[:, g].astype(np.uint8) << (5 - g))
    return fr


def records(pdt, ids, salt=11, t0=0.3125):
    """complete records whose counters are `ids` (the upper bits of byte 4 are noise), every other byte noise, every parity group passing"""
    n = len(ids)
    fr = np.zeros(n, dtype=pdt.FRAME_DTYPE)
    rng = np.random.default_rng(salt)
    body = rng.integers(0, 256, (n, 104)).astype(np.uint8)
    ids = np.asarray(ids, dtype=np.int64).reshape(n)
    body[:, 0], body[:, 1] = 0xED, 0xE2
    body[:, 4] = (body[:, 4] & 0xFE) | (ids >> 8).astype(np.uint8)
    body[:, 5] = (ids & 255).astype(np.uint8)
    fr["bytes"] = body
    fr["bit_index"] = 18 + 832 * np.arange(n)
    fr["time_src"] = 37 * np.arange(n)
    fr["time"] = t0 + np.arange(n) * 0.1 + np.arange(n) * 1e-7 / 3
    fr["nbytes"], fr["complete"] = 104, 1
    return fix_parity(fr)


def put(fr, byte, values, rows=None):
    """bytes[byte] of the records `rows` (all) = values, the parity groups mended behind it"""
    rows = np.arange(len(fr)) if rows is None else np.asarray(rows)
    fr["bytes"][rows, byte] = np.asarray(values, dtype=np.uint8)
    return fix_parity(fr)


def flip(fr, row, byte, bit=0x10):
    """one bit of a record complemented: the group that covers the byte now fails"""
    fr["bytes"][row, byte] ^= bit
    return fr


def hand_cases(pdt):
    """[dict(name, frames, table, trusted_only, thr)]: the hand-made cases"""
    sem, hk = listed_table(pdt, sem_list(), SEM_NAMES, 1), listed_table(pdt, HK_LIST, HK_NAMES, 0)
    cases = []

    def add(name, frames, tab=sem, trusted_only=False, thr=0):
        cases.append(dict(name=name, frames=frames, table=tab, trusted_only=trusted_only, thr=thr))

    add("no-records", records(pdt, []))
    add("one-record", records(pdt, [8]))
    add("one-record-nothing-fires", records(pdt, [12]), hk)
    add("sem-full-cycle", records(pdt, range(320)))
    add("hk-full-cycle", records(pdt, range(320)), hk)
    fr = records(pdt, [(7 + k) % 320 for k in range(60)])
    fr["complete"][20], fr["nbytes"][21], fr["complete"][22] = 0, 103, 2
    add("ineligible-in-the-middle", fr)
    fr = records(pdt, [8, 320, 8, 511, 28, 400])
    add("bad-ids", fr)
    # counters 8, 28, 48 ...: 9E1 (byte 20) and 9E2 (byte 21), both in group 1; group 0 holds the counter
    for trusted in (False, True):
        t = "-trusted" if trusted else ""
        add("group-0-fails" + t, flip(records(pdt, [8 + 20 * k for k in range(6)]), 2, 9), trusted_only=trusted)
        add("value-group-fails" + t, flip(records(pdt, [8 + 20 * k for k in range(6)]), 3, 25), trusted_only=trusted)
        add("both-fail" + t, flip(flip(records(pdt, [8 + 20 * k for k in range(6)]), 1, 9), 1, 21), trusted_only=trusted)
        add("hk-byte-in-group-0" + t, flip(records(pdt, [48, 128, 208]), 1, 11), hk, trusted_only=trusted)
    # bytes in no group: 0, 1, 87, 103; and the first and last covered ones, 2 and 86
    unc = table(pdt, [(0, 0, 1, 0, 0xFF, 0, 0), (1, 1, 1, 0, 0xFF, 0, 0), (2, 87, 1, 0, 0xFF, 0, 0), (3, 103, 1, 0, 0xFF, 0, 1), (4, 2, 1, 0, 0xFF, 0, 0),
                      (5, 86, 1, 0, 0xFF, 0, 0)])
    add("uncovered-bytes", flip(flip(records(pdt, [5, 6, 7, 8]), 1, 2), 2, 86), unc)
    add("uncovered-bytes-trusted", flip(flip(records(pdt, [5, 6, 7, 8]), 1, 2), 2, 86), unc, trusted_only=True)
    # a caller's table: channel 3 fed twice from one frame (entries 4 and 1, in that order of entry index: 1 first), unsorted, an empty channel 1
    own = table(pdt, [(5, 60, 4, 3, 0xFF, 0, 0), (3, 31, 2, 0, 0x7E, 1, 0), (0, 30, 1, 0, 0xFF, 0, 1), (2, 50, 5, 2, 0x0F, 0, 0), (3, 30, 2, 0, 0xFF, 0, 0),
                      (0, 44, 320, 7, 0xFF, 0, 0)])
    add("own-table", records(pdt, [(300 + k) % 320 for k in range(40)]), own)
    # spikes, on channel 0 of a one-entry table that fires in every record
    one = table(pdt, [(0, 30, 1, 0, 0xFF, 0, 0)])
    ids = list(range(10))
    add("spike", put(records(pdt, ids), 30, [100, 101, 140, 102, 103, 104, 80, 105, 106, 107]), one)
    add("spike-beside-spike", put(records(pdt, ids), 30, [100, 101, 140, 60, 103, 104, 104, 105, 106, 107]), one)
    add("first-and-last", put(records(pdt, ids), 30, [200, 101, 102, 103, 104, 105, 106, 107, 108, 10]), one)
    # single samples that stand 20, 21, 255 and 254 above a floor of zeros, under the thresholds 0 (= 20), 20, 21, 254 and 255
    v = [0, 20, 0, 0, 21, 0, 0, 255, 0, 0, 254, 0]
    for thr in (0, 20, 21, 254, 255):
        add(f"threshold-{thr}", put(records(pdt, range(12)), 30, v), one, thr=thr)
    # the spike test sees the values as decoded: inverted, masked and shifted
    nib = table(pdt, [(0, 30, 1, 0, 0xF0, 4, 1)])
    add("spike-on-decoded-values", put(records(pdt, ids), 30, [0xF0, 0xF1, 0x0F, 0xF2, 0xE0, 0xE1, 0xEF, 0xE2, 0xE3, 0xE4]), nib, thr=10)
    return cases


HAND_NAMES = (["no-records", "one-record", "one-record-nothing-fires", "sem-full-cycle", "hk-full-cycle", "ineligible-in-the-middle", "bad-ids"] +
              [n + t for t in ("", "-trusted") for n in ("group-0-fails", "value-group-fails", "both-fail", "hk-byte-in-group-0")] +
              ["uncovered-bytes", "uncovered-bytes-trusted", "own-table", "spike", "spike-beside-spike", "first-and-last"] +
              [f"threshold-{t}" for t in (0, 20, 21, 254, 255)] + ["spike-on-decoded-values"])


def seam_table(pdt):
    """channel 0: every record (byte 30); channel 2: two entries in every record whose counter ends a tile of 64 (bytes 41 and 40, in that
    order of entry index); channel 1 stays empty"""
    return table(pdt, [(0, 30, 1, 0, 0xFF, 0, 0), (2, 41, 64, 63, 0xFF, 0, 0), (2, 40, 64, 63, 0xFF, 0, 0)])


SEAM_NAMES = ["spike-left-of-seam", "spike-right-of-seam", "spikes-on-both-sides", "tile-without-usable-records", "tile-of-bad-ids", "all-at-once"]


def seam_cases(pdt, T):
    """[dict(name, frames, table, trusted_only, thr)]: 3 T records; the record's counter is its index, so the last record of every tile
    fires the two-entry channel, and channel 0's consecutive samples lie in different tiles"""
    assert T == 64
    cases = []
    tab = seam_table(pdt)

    def base(salt):
        fr = records(pdt, range(3 * T), salt=salt)
        return put(fr, 30, 100 + (np.arange(3 * T) % 7))            # a quiet series: no spike by itself

    def add(name, fr):
        cases.append(dict(name=name, frames=fr, table=tab, trusted_only=False, thr=0))

    add("spike-left-of-seam", put(base(1), 30, [200, 10], rows=[T - 1, 2 * T - 1]))
    add("spike-right-of-seam", put(base(2), 30, [200, 10], rows=[T, 2 * T]))
    add("spikes-on-both-sides", put(base(3), 30, [200, 20, 201, 19], rows=[T - 1, T, 2 * T - 1, 2 * T]))
    fr = put(base(4), 30, [200], rows=[T - 1])                      # its neighbours: T - 2 and, across a whole tile, 2 T
    fr["complete"][T:2 * T] = 0
    add("tile-without-usable-records", fr)
    fr = put(base(5), 30, [10], rows=[2 * T])
    fr["bytes"][T:2 * T, 4] |= 1
    fr["bytes"][T:2 * T, 5] |= 0x40                                 # counters 320 and up
    add("tile-of-bad-ids", fix_parity(fr))
    fr = put(base(6), 30, [200, 20, 10], rows=[T - 1, T, 2 * T])
    fr["nbytes"][T + 1:T + 9] = 100
    flip(fr, T - 1, 40)
    flip(fr, 2 * T - 1, 4, 0x02)
    add("all-at-once", fr)
    return cases


def big_table(pdt, seed=5):
    """256 entries over 128 channels, two each and unsorted: every period, covered and uncovered bytes, masks, shifts and inversions"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(256):
        period = int(rng.choice([1, 2, 4, 5, 8, 10, 16, 20, 32, 40, 64, 80, 160, 320]))
        byte = int(rng.choice([0, 1, 2, 11, 14, 18, 19, 20, 21, 35, 36, 52, 53, 69, 70, 86, 87, 102, 103]))
        shift = int(rng.integers(0, 8))
        rows.append((k % 128, byte, period, int(rng.integers(0, period)), int(rng.integers(1, 256)), shift, int(rng.integers(0, 2))))
    order = rng.permutation(256)
    return table(pdt, [rows[k] for k in order])


def kind4_records(pdt, nframes, first=0, flips=0, seed=7):
    """the frames first .. first + nframes - 1 a kind 4 capture carries, as records; `flips` bits complemented here and there -- not in the
    counter's bytes 4 and 5 -- so that parity groups fail"""
    p = pdt.synth_params(4, 50000, 1000.0, seed)
    fr = np.zeros(nframes, dtype=pdt.FRAME_DTYPE)
    for k in range(nframes):
        fr["bytes"][k] = pdt.synth_poes_frame(p, first + k)
    fr["bit_index"] = 18 + 832 * np.arange(nframes)
    fr["time"] = 0.0125 + np.arange(nframes) * 0.1
    fr["nbytes"], fr["complete"] = 104, 1
    rng = np.random.default_rng(seed + 100)
    for _ in range(flips):
        fr["bytes"][int(rng.integers(0, nframes)), int(rng.choice([2, 3] + list(range(6, 104))))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return fr


def format_py(samples, names=None):
    """the samples' text with Python's %"""
    out = b""
    for r in samples:
        c = int(r["channel"])
        name = names[c] if names is not None and c < len(names) else "c%u" % c
        fl = "".join(ch for bit, ch in ((1, "b"), (2, "i"), (4, "u"), (8, "s")) if int(r["flags"]) & bit) or "-"
        out += ("%.5f %s %u %u %s\n" % (float(r["time"]), name, int(r["minor_id"]), int(r["value"]), fl)).encode()
    return out
