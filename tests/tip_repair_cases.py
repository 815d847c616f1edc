"""Cases for the repair of failed TIP parity groups, and a plain-Python statement of the rule written from the text of
include/pdt.h: which records are checked, frame bit j and its soft value, the five groups and their parity bits, the candidates (group
0 without frame bits 16 - 18), r = the bit pattern of |soft| with NaN as 0, the key (r << 16) | j, the complement of the smallest key in
a failing group, and the info record.  A case is a dict: name, soft (float32[n]), frames (FRAME_DTYPE[k]) and, where the outcome was
derived by hand, want_failed / want_pos / want_status / want_bytes per record."""
import ctypes as C

import numpy as np

NONE = 0xFFFF
N_COVERED = 685


def group_bits(g):
    """the 137 frame bits of group g: 136 data bits, then the parity bit"""
    return list(range(16 + 136 * g, 152 + 136 * g)) + [826 + g]


def candidates(g):
    return [j for j in group_bits(g) if j > 18]


COVERED = np.array(sorted(j for g in range(5) for j in group_bits(g)))
assert len(COVERED) == N_COVERED


def get_bit(b, j):
    return (int(b[j >> 3]) >> (7 - (j & 7))) & 1


def flip_bit(b, j):
    b[j >> 3] ^= 0x80 >> (j & 7)


def failing(b):
    """bit g set where group g of the 104 bytes has odd parity"""
    return sum((sum(get_bit(b, j) for j in group_bits(g)) & 1) << g for g in range(5))


def frame_bits(b):
    return np.unpackbits(np.asarray(b, dtype=np.uint8))


def checked(rec, n):
    return int(rec["complete"]) == 1 and int(rec["nbytes"]) == 104 and 18 <= int(rec["bit_index"]) and int(rec["bit_index"]) + 813 < n


def model(pdt, soft, frames):
    """the rule, record by record: (repaired copy, info, summary dict)"""
    soft = np.ascontiguousarray(soft, dtype="<f4").reshape(-1)
    r = soft.view("<u4") & 0x7FFFFFFF
    r = np.where(r > 0x7F800000, 0, r).astype(np.uint64)
    out = np.array(frames, dtype=pdt.FRAME_DTYPE, copy=True).reshape(-1)
    info = np.zeros(len(out), dtype=pdt.TIP_REPAIR_INFO_DTYPE)
    sm = dict(checked=0, skipped=0, failing=0, repaired=0)
    for f in range(len(out)):
        info[f]["pos"][:] = NONE
        if not checked(out[f], len(soft)):
            sm["skipped"] += 1
            continue
        info[f]["status"] = 1
        sm["checked"] += 1
        b, p = out[f]["bytes"], int(out[f]["bit_index"])
        fails, flips = failing(b), []
        for g in range(5):
            keys = sorted((int(r[p - 18 + j]) << 16) | j for j in candidates(g))
            info[f]["least"][g] = np.array([keys[0] >> 16], dtype="<u4").view("<f4")[0]
            info[f]["next"][g] = np.array([keys[1] >> 16], dtype="<u4").view("<f4")[0]
            if fails >> g & 1:
                info[f]["pos"][g] = keys[0] & 0xFFFF
                flips.append(keys[0] & 0xFFFF)
        for j in flips:
            flip_bit(b, j)
        info[f]["failed"] = fails
        sm["failing"] += 1 if fails else 0
        sm["repaired"] += len(flips)
    return out, info, sm


def same(got, want):
    """records, info and summary byte for byte"""
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


def good_frame(pdt, rng, p, inverted=0):
    """a record at bit_index p whose five groups pass"""
    rec = np.zeros(1, dtype=pdt.FRAME_DTYPE)[0]
    b = rng.integers(0, 256, 104).astype(np.uint8)
    b[0], b[1], b[2] = 0xED, 0xE2, b[2] & 0x1F
    for g in range(5):
        if failing(b) >> g & 1:
            flip_bit(b, 826 + g)
    rec["time"], rec["bit_index"], rec["time_src"], rec["inverted"], rec["nbytes"], rec["complete"] = p / 8320.0, p, 6 * p, inverted, 104, 1
    rec["bytes"] = b
    return rec


def soft_stream(rng, n):
    """magnitudes in [1, 2), random signs: every |value| the cases set below 1 is the smallest"""
    return ((1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)).astype("<f4")


def _case(name, soft, frames, **want):
    return dict(name=name, soft=np.asarray(soft, dtype="<f4"), frames=np.array(frames), **want)


def hand_cases(pdt):
    rng = np.random.default_rng(23)
    D = pdt.FRAME_DTYPE
    cases = []

    def one(p=100, n=2000, inverted=0):
        return soft_stream(rng, n), good_frame(pdt, rng, p, inverted)

    # one failing group, g = 0 .. 4: a data bit is wrong and is the least reliable
    for g in range(5):
        soft, rec = one()
        want = rec["bytes"].copy()
        j = 16 + 136 * g + 50 + g
        flip_bit(rec["bytes"], j)
        soft[100 - 18 + j] = np.float32(0.25) * (1 if get_bit(rec["bytes"], j) else -1)
        cases.append(_case(f"group-{g}", soft, np.array([rec], dtype=D), want_failed=[1 << g], want_pos=[[j if k == g else NONE for k in range(5)]],
                           want_bytes=[want], want_status=[1]))
    # all five groups fail in one frame
    soft, rec = one()
    want, js = rec["bytes"].copy(), [19, 160, 423, 559, 695]
    for j in js:
        flip_bit(rec["bytes"], j)
        soft[82 + j] = 0.125
    cases.append(_case("all-five", soft, np.array([rec], dtype=D), want_failed=[31], want_pos=[js], want_bytes=[want], want_status=[1]))
    # the minimum on the parity bit: five wavefronts meet in byte 103
    soft, rec = one()
    want = rec["bytes"].copy()
    for g in range(5):
        flip_bit(rec["bytes"], 826 + g)
        soft[82 + 826 + g] = -0.5
    cases.append(_case("parity-bits", soft, np.array([rec], dtype=D), want_failed=[31], want_pos=[[826 + g for g in range(5)]], want_bytes=[want],
                       want_status=[1]))
    # the minimum on group 0's excluded bits: the sync word's last three are never chosen, however unreliable
    soft, rec = one()
    want = rec["bytes"].copy()
    flip_bit(rec["bytes"], 40)
    soft[82 + 16:82 + 19] = [0.0, 1e-20, -1e-30]
    soft[82 + 40] = 0.75
    cases.append(_case("excluded-bits", soft, np.array([rec], dtype=D), want_failed=[1], want_pos=[[40, NONE, NONE, NONE, NONE]], want_bytes=[want],
                       want_status=[1]))
    # the excluded bits count toward the parity: a record whose bit 17 is set fails group 0
    soft, rec = one()
    flip_bit(rec["bytes"], 17)
    soft[82 + 17] = 0.0
    soft[82 + 151] = 0.5
    want = rec["bytes"].copy()
    flip_bit(want, 151)
    cases.append(_case("excluded-bit-set", soft, np.array([rec], dtype=D), want_failed=[1], want_pos=[[151, NONE, NONE, NONE, NONE]], want_bytes=[want],
                       want_status=[1]))
    # ties: the earlier bit; a data bit before the parity bit; a stream of equal values: each group's first candidate
    soft, rec = one()
    want = rec["bytes"].copy()
    flip_bit(rec["bytes"], 200)
    flip_bit(rec["bytes"], 287 + 136)
    soft[82 + 200], soft[82 + 250], soft[82 + 170 + 136] = 0.5, -0.5, 0.5
    soft[82 + 287 + 136], soft[82 + 828] = 0.5, -0.5
    flip_bit(want, 423)
    flip_bit(want, 306)          # (group 1: 200 before 250, repaired; group 2: 306 before 423 and the parity bit 828 -- two wrong bits now)
    cases.append(_case("ties", soft, np.array([rec], dtype=D), want_failed=[0b110], want_pos=[[NONE, 200, 306, NONE, NONE]],
                       want_bytes=[want], want_status=[1]))
    soft, rec = one()
    soft[:] = -3.0
    for g in range(5):
        flip_bit(rec["bytes"], 100 + 136 * g)
    want = rec["bytes"].copy()
    firsts = [19, 152, 288, 424, 560]
    for j in firsts:
        flip_bit(want, j)
    cases.append(_case("all-equal", soft, np.array([rec], dtype=D), want_failed=[31], want_pos=[firsts], want_bytes=[want], want_status=[1]))
    # NaN counts as 0, -0 as 0, Inf above every finite value
    soft, rec = one()
    want = rec["bytes"].copy()
    for j in (30, 200, 300, 450, 600):
        flip_bit(rec["bytes"], j)
    soft[82 + 30], soft[82 + 25] = np.nan, 1e-38                           # group 0: the NaN is 0, below the smallest normal
    soft[82 + 200], soft[82 + 190] = -0.0, np.float32(1e-45)               # group 1: -0 below the smallest subnormal
    soft[82 + 300], soft[82 + 310] = -np.nan, 0.0                          # group 2: NaN and 0 tie, the earlier bit
    for j in candidates(3):
        soft[82 + j] = np.inf if j & 1 else -np.inf
    soft[82 + 450] = 3.0e38                                                # group 3: the one finite value
    for j in candidates(4):
        soft[82 + j] = -np.inf                                             # group 4: all Inf, the first candidate
    flip_bit(want, 600)
    flip_bit(want, 560)
    cases.append(_case("nan-inf-zero", soft, np.array([rec], dtype=D), want_failed=[31], want_pos=[[30, 200, 300, 450, 560]], want_bytes=[want],
                       want_status=[1]))
    # an inverted record: the bytes are already complemented back, the field plays no part
    soft, rec = one(inverted=1)
    want = rec["bytes"].copy()
    flip_bit(rec["bytes"], 500)
    soft[82 + 500] = 0.001
    cases.append(_case("inverted", soft, np.array([rec], dtype=D), want_failed=[8], want_pos=[[NONE, NONE, NONE, 500, NONE]], want_bytes=[want],
                       want_status=[1]))
    # the first record of a stream (bit_index 18, its group 0 reads from soft value 19) and the last (ending at n - 1)
    n = 18 + 832 + 829
    soft = soft_stream(rng, n)
    a, b = good_frame(pdt, rng, 18), good_frame(pdt, rng, n - 814)
    wa, wb = a["bytes"].copy(), b["bytes"].copy()
    flip_bit(a["bytes"], 19)
    flip_bit(b["bytes"], 830)
    soft[19], soft[n - 1], soft[n - 2] = 0.5, 0.5, 0.25
    cases.append(_case("stream-ends", soft, np.array([a, b], dtype=D), want_failed=[1, 16], want_pos=[[19] + [NONE] * 4, [NONE] * 4 + [830]],
                       want_bytes=[wa, wb], want_status=[1, 1]))
    # skipped: bit_index 17, bit_index + 813 == n, complete 0, nbytes 103 -- left as they are, failing groups and all
    n = 3000
    soft = soft_stream(rng, n)
    recs = [good_frame(pdt, rng, 17), good_frame(pdt, rng, n - 813), good_frame(pdt, rng, 500), good_frame(pdt, rng, 500), good_frame(pdt, rng, -5),
            good_frame(pdt, rng, 500)]
    recs[2]["complete"], recs[3]["nbytes"] = 0, 103
    for r in recs:
        flip_bit(r["bytes"], 300)
    want = [r["bytes"].copy() for r in recs]
    soft[482 + 300] = 0.5
    flip_bit(want[5], 300)
    cases.append(_case("skipped", soft, np.array(recs, dtype=D), want_failed=[0, 0, 0, 0, 0, 4], want_pos=[[NONE] * 5] * 5 + [[NONE, NONE, 300, NONE, NONE]],
                       want_bytes=want, want_status=[0, 0, 0, 0, 0, 1]))
    # two records that overlap by three bits: frame bits 829 - 831 of the first are frame bits 0 - 2 of the second
    n = 100 + 829 + 900
    soft = soft_stream(rng, n)
    a, b = good_frame(pdt, rng, 100), good_frame(pdt, rng, 929)
    wa, wb = a["bytes"].copy(), b["bytes"].copy()
    flip_bit(a["bytes"], 829)
    flip_bit(a["bytes"], 830)
    flip_bit(b["bytes"], 19)
    soft[82 + 829], soft[82 + 830], soft[82 + 831], soft[911 + 19] = 0.5, -0.5, 0.0, 0.5
    cases.append(_case("overlap-3", soft, np.array([a, b], dtype=D), want_failed=[24, 1], want_pos=[[NONE] * 3 + [829, 830], [19] + [NONE] * 4],
                       want_bytes=[wa, wb], want_status=[1, 1]))
    # n = 0: no records; and records against an empty stream
    cases.append(_case("no-records", soft_stream(rng, 1000), np.zeros(0, dtype=D)))
    cases.append(_case("no-soft", np.zeros(0, dtype="<f4"), np.array([good_frame(pdt, rng, 100)], dtype=D), want_failed=[0], want_pos=[[NONE] * 5],
                       want_status=[0]))
    return cases


def random_case(pdt, count=300, seed=2023):
    """records of random bytes -- about half of their groups fail -- on random soft values with zeros, NaN, Inf and ties among them; every
    tenth record is one the rule skips"""
    rng = np.random.default_rng(seed)
    n = 18 + 832 * count + 400
    soft = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e3], n)).astype("<f4")
    soft[rng.integers(0, n, n // 50)] = rng.choice(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, -0.5], dtype="<f4"), n // 50)
    recs = np.zeros(count, dtype=pdt.FRAME_DTYPE)
    for f in range(count):
        p = 18 + 832 * f + int(rng.integers(0, 400))
        recs[f] = good_frame(pdt, rng, p, int(rng.integers(0, 2)))
        recs[f]["bytes"] = rng.integers(0, 256, 104).astype(np.uint8)
        if f % 10 == 9:
            k = int(rng.integers(0, 4))
            if k == 0:
                recs[f]["complete"] = 0
            elif k == 1:
                recs[f]["nbytes"] = int(rng.integers(0, 104))
            elif k == 2:
                recs[f]["bit_index"] = int(rng.integers(-5, 18))
            else:
                recs[f]["bit_index"] = n - 813 + int(rng.integers(0, 900))
    return dict(name="random-300", soft=soft, frames=recs)


def weak_capture(pdt, kind=3, mult=9.0, seed=1234, seconds=30.0, fs=50000):
    """test_tip_sync.weak_capture with the frames of `kind`"""
    p = pdt.synth_params(kind, fs, 1000.0, seed)
    p.noise_gain = int(round(p.noise_gain * mult))
    x = np.zeros((int(round(seconds * fs)), 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, len(x), x.ctypes.data)
    return p, x


def covered_errors(pdt, p, before, after, nsent):
    """Records against the frames the generator sent, over the 685 bits the five groups cover.  A record belongs to the sent frame its
    bytes as decoded are nearest to; it is placed when that is within 100 bits.  Returns (placed, frames without a wrong covered bit
    before and after the repair, wrong covered bits before and after)."""
    if len(before) == 0:
        return 0, 0, 0, 0, 0
    sent = np.stack([frame_bits(pdt.synth_poes_frame(p, k))[COVERED] for k in range(nsent)])
    placed = clean0 = clean1 = wrong0 = wrong1 = 0
    for b0, b1 in zip(before, after):
        d = (sent ^ frame_bits(b0["bytes"])[COVERED]).sum(axis=1)
        k = int(d.argmin())
        if d[k] > 100:
            continue
        e = int((sent[k] ^ frame_bits(b1["bytes"])[COVERED]).sum())
        placed, clean0, clean1, wrong0, wrong1 = placed + 1, clean0 + (d[k] == 0), clean1 + (e == 0), wrong0 + int(d[k]), wrong1 + e
    return placed, int(clean0), int(clean1), wrong0, wrong1


def ffp_frames_host(pdt, rate, x):
    """an int16 capture through host_ffp_bits and host_tip_sync: (the bits record, the frames)"""
    got = pdt.host_ffp_bits(rate, np.asarray(x).astype(np.float32) / np.float32(32768.0))
    return got, pdt.host_tip_sync(got.bits.tobytes())


def golden_clip_frames(golden_dir):
    import os
    text = open(os.path.join(golden_dir, "clip.c10000.txt")).read().split("\n")
    want = [bytes(int(h, 16) for h in line.split()[1:]) for line in text if len(line.split()) == 105]
    assert len(want) == 47
    return want
