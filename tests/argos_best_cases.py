"""Bit strings and captures for the tests of the ARGOS messages' second rule, PDT_ARGOS_RULE_BEST (a plain module beside
argos_msg_cases.py, no fixtures here), shared by tests/test_argos_best.py (the host restatement against a Python model),
tests/test_gpu_argos_best.py (the kernels against the host restatement) and tools/argos_rule_survey.py.  Strings are bytes of '0'/'1';
a case is (name, string, min_run)."""
import ctypes as C

import numpy as np

from argos_msg_cases import CODES, SYNC, at_seams, body, crafted, data_for, flip, message, random_bits
from test_windows import ARGOS_RANGE, D, FS, IN_RATE, OFFSETS, PERIOD_S, RESIDUAL

NOISE = "0110100110010110"                               # no sync, no run longer than two


def exact(n: int, ident: int, data: bytes, inverted: int, rv: str, run: int, stray: str = "") -> str:
    """a message whose run is exactly `run` bits of `rv` (the other value in front of it), then `stray`, then sync, code and body"""
    return flip(rv) + message(n, ident, data, inverted, rv * run + stray)


def data_of(bits: str, n: int) -> bytes:
    """`bits` at the start of the 32 n data bits of a message, the rest NOISE"""
    s = (bits + NOISE * (2 * n + 1))[: 32 * n]
    assert len(bits) <= 32 * n
    return bytes(int(s[i: i + 8], 2) for i in range(0, 32 * n, 8))


def nested(outer_run: int, outer_stray: str, inner_run: int, inner_stray: str, inv_outer: int = 0, inv_inner: int = 0) -> str:
    """an eight-block message (ID 0AAAA) with a one-block message (ID 0BBBB) inside its data: the runs' lengths and stray bits choose
    which of the two a rule accepts"""
    inner = exact(1, 0x0BBBB, data_for(1, 3), inv_inner, "1", inner_run, inner_stray)
    payload = NOISE + inner
    if inv_outer:
        payload = flip(payload)                          # (the outer body is written in the outer's polarity: the raw bits stay `inner`)
    return NOISE + exact(8, 0x0AAAA, data_of(payload, 8), inv_outer, "0", outer_run, outer_stray) + NOISE


def overlay(length: int, parts) -> str:
    """filler "01" with every (start, string) of `parts` written over it, in order"""
    s = list(("01" * (length // 2 + 1))[:length])
    for start, part in parts:
        assert 0 <= start and start + len(part) <= length
        s[start: start + len(part)] = part
    return "".join(s)


def chain(runs) -> str:
    """heads A (2 blocks), B (3 blocks) and C (1 block) with exactly `runs` equal bits each: B's head lies in A's body, C's in B's
    body behind A's last bit, so A and B overlap, B and C overlap, A and C do not.  IDs 0000A, 0000B, 0000C."""
    ra, rb, rc_ = runs
    a, b, c = (exact(n, i, data_of("", n), 0, "1", r) for n, i, r in ((2, 0x0000A, ra), (3, 0x0000B, rb), (1, 0x0000C, rc_)))
    ea = 100                                             # A's length code ends here; its span ends at ea + 84
    start_a = ea - 12 - ra - 1
    start_b = ea + 40 - rb - 1                           # B's sync begins at ea + 40: eB = ea + 52, its span ends at ea + 168
    start_c = ea + 94 - rc_ - 1                          # C's sync begins at ea + 94, behind A's last bit ea + 84
    return overlay(500, ((start_a, a), (start_b, b), (start_c, c)))


def crafted_best():
    """(name, string, min_run) of the new crafted cases of rule 1"""
    cases = []
    for k in (0, 1, 6, 15):
        for inv in (0, 1):
            for rv in "01":
                for stray in "01":
                    # fifteen run bits, one bit of either value, the sync (K = 0: s stays 0)
                    cases.append((f"stray{stray}-K{k}-inv{inv}-run{rv}", NOISE + exact(2, 0x1F00D, data_for(2, k + 1), inv, rv, 15, stray) + NOISE, k))
                if k < 2:
                    continue                             # (any single bit is a run of one: the cases below need K >= 2)
                stray = flip(rv)
                # exactly K run bits behind the stray bit, and K - 1
                cases.append((f"K{k}-slip-exact-inv{inv}-run{rv}", NOISE + exact(2, 0x0F0F0, data_for(2, k), inv, rv, k, stray) + NOISE, k))
                cases.append((f"K{k}-slip-short-inv{inv}-run{rv}", NOISE + exact(2, 0x0F0F0, data_for(2, k), inv, rv, k - 1, stray) + NOISE, k))
                # the head at e = 12 + K + 1 with s = 1, and one bit less
                cases.append((f"K{k}-slip-first-inv{inv}-run{rv}", message(3, 0x54321, data_for(3, k), inv, rv * k + stray) + NOISE, k))
                cases.append((f"K{k}-slip-before-first-inv{inv}-run{rv}", message(3, 0x54321, data_for(3, k), inv, rv * (k - 1) + stray) + NOISE, k))
    # both s = 0 and s = 1 hold: sixteen equal bits
    for rv in "01":
        cases.append((f"both-slips-run{rv}", NOISE + message(1, 0x2B0B0, data_for(1, 4), 0, rv * 16) + NOISE, 6))
    # a false eight-block head with a run of 6 and the true head with a run of 15 inside its body; the roles reversed; equal scores
    for io in (0, 1):
        for ii in (0, 1):
            cases.append((f"false-outer-inv{io}{ii}", nested(6, "", 15, "", io, ii), 6))
            cases.append((f"false-inner-inv{io}{ii}", nested(15, "", 6, "", io, ii), 6))
            cases.append((f"equal-score-inv{io}{ii}", nested(6, "", 6, "", io, ii), 6))
    # s = 0 beats s = 1 at equal run_len, whichever of the two lies in front
    cases.append(("slip-loses-outer", nested(10, "1", 10, ""), 6))
    cases.append(("slip-loses-inner", nested(10, "", 10, "0"), 6))
    # the chain: scores C > B > A, and B highest
    cases.append(("chain-CBA", chain((2, 4, 8)), 2))
    cases.append(("chain-B", chain((2, 8, 4)), 2))
    # a head inside an accepted body (its run is the longer one this time: it wins) followed by one just behind the outer body
    inner = "1" * 15 + SYNC + CODES[0] + body(1, 0x0D0D0, data_for(1, 2))
    payload = NOISE[:3] + "0" + inner
    outer = exact(4, 0x33333, data_of(payload, 4)[:-1] + b"\x00", 0, "1", 6)
    cases.append(("inside-strong", NOISE + outer + message(1, 0x44444, data_for(1, 8), 0, "") + NOISE, 6))
    cases.append(("capped-cluster", "0001011110000" * 320, 0))
    # ... and where the cap decides: 256 heads fill a cluster, the 257th has the longest run of all (17 zeros in front of its sync) and
    # overlaps the last one accepted, so it is struck; without the cap it would win and strike that one
    cases.append(("capped-cluster-decides", "0000" + "0001011110000" * 256 + "0" * 13 + "0001011110000" * 10, 0))
    cases.append(("empty", "", 6))
    cases.append(("twelve", "000101111000", 0))
    return [(name, s.encode(), k) for name, s, k in cases]


def long_random() -> bytes:
    """200 000 random bits: more than 256 accepted messages at K = 0"""
    return random_bits(200000, 11)


def existing(tile: int):
    """every string of argos_msg_cases at K in (0, 1, 6, 15)"""
    out = []
    for name, bits, _ in crafted() + at_seams(tile):
        out += [(f"{name}@K{k}", bits, k) for k in (0, 1, 6, 15)]
    out += [(f"random@K{k}", random_bits(), k) for k in (0, 1, 6, 15)]
    return out


def best_seams(tile: int, limit: int = 9000):
    """(name, string, min_run): at every seam k * tile below `limit`, and at the pick kernel's tile-group boundary 64 * tile, at offsets
    -1, 0 and +1: a head with a stray bit whose length code ends there; a cluster (a false outer head, the true one inside its body)
    whose inner head ends there, and one whose outer head ends there"""
    cases = []
    seams = [k * tile for k in range(1, (limit - 1) // tile + 1)] + [64 * tile]
    inner_at = nested(6, "", 15, "").index("1" * 15 + SYNC) + 15 + 12          # the inner head's e within the string nested() gives
    outer_at = len(NOISE) + 1 + 6 + 12
    for seam in seams:
        for d in (-1, 0, 1):
            e = seam + d
            m = exact(2, 0x5A5A5, data_for(2, d + 2), seam & 1, "0", 15, "1")
            cases.append((f"seam{seam}{d:+d}-stray", overlay(e + 300, ((e - 12 - 17, m),)), 6))
            for name, at in (("inner", inner_at), ("outer", outer_at)):
                s = nested(6, "", 15, "")
                cases.append((f"seam{seam}{d:+d}-cluster-{name}", overlay(e + 500, ((e - at, s),)), 6))
    return [(name, s.encode(), k) for name, s, k in cases]


# ---------------------------------------------------------------- two kind-2 platforms in a wideband capture, cut into windows
def kind2_pair(pdt, seeds, secs: float):
    """test_argos_messages.kind2_platforms at the seeds asked for"""
    n = int(round(secs * IN_RATE))
    total = np.zeros((n, 2), dtype=np.int32)
    params = []
    for off, seed in zip(OFFSETS, seeds):
        p = pdt.synth_params(2, IN_RATE, off + RESIDUAL, seed)
        p.amplitude //= 2
        p.noise_gain //= 2
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
        total += iq
        params.append(p)
    return np.clip(total, -32768, 32767).astype(np.int16), params


def sent_for_window(pdt, params, w):
    near = int(np.argmin([abs(w.offset_hz - (off + RESIDUAL)) for off in OFFSETS]))
    n, i, d = pdt.synth_argos_message(params[near], int(round(w.first_frame / IN_RATE / PERIOD_S)))
    return n, i, bytes(d)


def decoded(m):
    return [(int(r["blocks"]), int(r["id"]), bytes(r["data"][: 4 * r["blocks"]])) for r in m if r["complete"]]


def host_window_bits(pdt, orc, x, math_mode=None):
    """host_bursts -> burst_windows -> host_ddc of each slice -> the oracle's bits: (windows, one bit string per window)"""
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, rows=False)
    win = pdt.burst_windows(found, IN_RATE, len(x))
    bits = []
    for w in win:
        y = pdt.host_ddc(IN_RATE, D, w.offset_hz, x[w.first_frame: w.first_frame + w.nframes])
        y16 = np.clip(np.round(y.reshape(-1, 2) * 32768.0), -32768, 32767).astype(np.int16)
        o = orc.Oracle(orc.ARGOS, FS, y16) if math_mode is None else orc.Oracle(orc.ARGOS, FS, y16, math_mode=math_mode)
        bits.append(o.stage(orc.ST_BITS).tobytes())
    return win, bits


def tally(pdt, params, windows, messages):
    """(right, wrong, lost frames): windows whose decoded messages are exactly the one sent for their burst; windows that hold a
    message other than it; the first frames of the windows that are not right"""
    right = wrong = 0
    lost = []
    for w, m in zip(windows, messages):
        sent, got = sent_for_window(pdt, params, w), decoded(m)
        right += got == [sent]
        wrong += any(g != sent for g in got)
        if got != [sent]:
            lost.append(int(w.first_frame))
    return right, wrong, lost
