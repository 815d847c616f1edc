"""Bit strings for the flywheel frame synchroniser, shared by the CPU and the GPU tests: a statement of the rule in plain
Python written from its text (include/pdt.h), a builder that plants sync words into a string, the hand-derived cases with their expected
records written out, 200 random strings, and the strings that put things on the seams of the kernels' tiles."""
import numpy as np

S = "1110110111100010000"
F = 832
BODY = 813                      # bits behind p a whole frame needs
DEFAULTS = (2, 2, 3)            # E = max_errors, W = window, G = fly


def model(bits: bytes, E: int = 2, W: int = 2, G: int = 3):
    """The rule from its text: a list of dicts in ascending p -- bit_index, inverted, sync_errors, support, candidate, bytes."""
    b = np.array([0 if v == ord("0") else 1 for v in bytes(bits)], dtype=np.int64)
    n = len(b)
    if n < 19:
        return []
    sync = np.array([int(c) for c in S], dtype=np.int64)
    plus = np.zeros(n, dtype=np.int64)                       # dist+(p), p >= 18
    for j in range(19):
        plus[18:] += b[j: n - 18 + j] != sync[j]

    def dist(p, s):
        return int(19 - plus[p] if s else plus[p])

    pos = np.arange(n) >= 18
    heads = {}
    for s in (0, 1):
        cand = pos & ((19 - plus if s else plus) <= E)        # c_s(p); no position below 18 or behind the stream
        u = np.zeros(n, dtype=np.int64)                       # u_s(p): the candidates at p + k F, k = -W .. -1, 1 .. W
        for k in range(1, W + 1):
            if k * F < n:
                u[: n - k * F] += cand[k * F:]
                u[k * F:] += cand[: n - k * F]
        is_head = pos & (np.arange(n) + BODY < n) & ((cand & (u >= 1)) | (u >= G))
        for p in np.nonzero(is_head)[0]:
            p = int(p)
            key = (int(u[p]), int(cand[p]), -dist(p, s))
            if p not in heads or key > heads[p][0]:           # (the upright one came first: it stands at equal keys)
                heads[p] = (key, s)
    order = sorted(heads)
    out = []
    for p in order:
        key, s = heads[p]
        rivals = [g for g in order if g != p and abs(g - p) <= F - 4]
        if any(heads[g][0] > key or (heads[g][0] == key and g < p) for g in rivals):
            continue
        out.append(dict(bit_index=p, inverted=s, sync_errors=dist(p, s), support=key[0], candidate=key[1], bytes=frame_bytes(bits, p, s)))
    return out


def frame_bytes(bits: bytes, p: int, inv: int) -> bytes:
    """the 104 bytes of the frame whose sync word completes at p, as the reference prints them"""
    v = [(0 if c == ord("0") else 1) ^ inv for c in bytes(bits[p + 1: p + 1 + BODY])]
    assert len(v) == BODY
    first = int("".join(map(str, v[:5])), 2)
    rest = [int("".join(map(str, v[5 + 8 * j: 13 + 8 * j])), 2) for j in range(101)]
    return bytes([0xED, 0xE2, first] + rest)


def plant(n: int, words, seed: int = 1, fill: str = "payload") -> bytes:
    """A string of n bits, zeros, with sync words planted: words = (p, inverted, flipped offsets 0 .. 18 of the word) -- the word
    completes at bit p.  fill 'payload': the 813 bits behind every planted word are random (seeded) first, so that the frames' bytes say
    something; planted words overwrite payload."""
    rng = np.random.default_rng(seed)
    b = np.zeros(n, dtype=np.uint8)
    if fill == "payload":
        for p, _, _ in words:
            lo, hi = max(p + 1, 0), min(p + 1 + BODY, n)
            if hi > lo:
                b[lo:hi] = rng.integers(0, 2, hi - lo)
    for p, inv, flips in words:
        w = [int(c) ^ inv for c in S]
        for k in flips:
            w[k] ^= 1
        for j in range(19):
            i = p - 18 + j
            if 0 <= i < n:
                b[i] = w[j]
    return bytes(b + ord("0"))


def rec(p, inv, d, u, c):
    return dict(bit_index=p, inverted=inv, sync_errors=d, support=u, candidate=c)


P0 = 100
A3 = 18 + 2 * F + 50            # the three-head chain's A


def cases():
    """(name, bits, cfg or None, expected records) -- the expectations are derived by hand from the rule's text, at its defaults unless a
    cfg = (E, W, G) stands; bytes are those of the string at the expected position"""
    out = []
    n2 = P0 + F + BODY + 40
    # dist exactly E: a chain of two, the second with two wrong bits -- both are candidates, each the other's support
    out.append(("dist_E", plant(n2, [(P0, 0, ()), (P0 + F, 0, (3, 11))]), None, [rec(P0, 0, 0, 1, 1), rec(P0 + F, 0, 2, 1, 1)]))
    # dist E + 1: the second is no candidate; with u = 1 < G it is no head, and the first has lost its support
    out.append(("dist_E_plus_1", plant(n2, [(P0, 0, ()), (P0 + F, 0, (3, 11, 17))]), None, []))
    # a candidate alone: u = 0, no head
    out.append(("candidate_u0", plant(n2, [(P0, 0, ())]), None, []))
    # ... and with one neighbour: u = 1, heads both
    out.append(("candidate_u1", plant(n2, [(P0, 0, ()), (P0 + F, 0, ())]), None, [rec(P0, 0, 0, 1, 1), rec(P0 + F, 0, 0, 1, 1)]))
    # a slot whose own word is destroyed (8 wrong bits) between slots 0, 1 and nothing behind: u = 2 = G - 1, none
    n5 = P0 + 4 * F + BODY + 40
    broken = (0, 2, 4, 6, 8, 10, 12, 14)
    out.append(("flywheel_G_minus_1", plant(n5, [(P0, 0, ()), (P0 + F, 0, ()), (P0 + 2 * F, 0, broken)]), None,
                [rec(P0, 0, 0, 1, 1), rec(P0 + F, 0, 0, 1, 1)]))
    # ... with slot 3 as well: u = 3 = G, a flywheel head: candidate 0, 8 sync errors, bytes as the stream holds them
    out.append(("flywheel_G", plant(n5, [(P0, 0, ()), (P0 + F, 0, ()), (P0 + 2 * F, 0, broken), (P0 + 3 * F, 0, ())]), None,
                [rec(P0, 0, 0, 1, 1), rec(P0 + F, 0, 0, 2, 1), rec(P0 + 2 * F, 0, 8, 3, 0), rec(P0 + 3 * F, 0, 0, 1, 1)]))
    # an inverted chain of three, one wrong bit in the middle one
    out.append(("inverted_chain", plant(n5, [(P0, 1, ()), (P0 + F, 1, (9,)), (P0 + 2 * F, 1, ())]), None,
                [rec(P0, 1, 0, 2, 1), rec(P0 + F, 1, 1, 2, 1), rec(P0 + 2 * F, 1, 0, 2, 1)]))
    # an inverted flywheel head between upright-looking damage: slots 0, 1, 3 inverted, slot 2 destroyed
    out.append(("inverted_flywheel", plant(n5, [(P0, 1, ()), (P0 + F, 1, ()), (P0 + 2 * F, 1, broken), (P0 + 3 * F, 1, ())]), None,
                [rec(P0, 1, 0, 1, 1), rec(P0 + F, 1, 0, 2, 1), rec(P0 + 2 * F, 1, 8, 3, 0), rec(P0 + 3 * F, 1, 0, 1, 1)]))
    # the neighbour exists only at p - F: the last frame of a stream
    out.append(("neighbour_behind_only", plant(n2, [(P0, 0, ()), (P0 + F, 0, ())]), None, [rec(P0, 0, 0, 1, 1), rec(P0 + F, 0, 0, 1, 1)]))
    # the neighbour at p - F = 17 < 18 is no position: the word at 17 + F has no support
    out.append(("neighbour_at_17", plant(17 + F + BODY + 40, [(17, 0, ()), (17 + F, 0, ())]), None, []))
    # ... at 18 it is one, and a head itself
    out.append(("neighbour_at_18", plant(18 + F + BODY + 40, [(18, 0, ()), (18 + F, 0, ())]), None, [rec(18, 0, 0, 1, 1), rec(18 + F, 0, 0, 1, 1)]))
    # p + 813 = n - 1: the last frame is whole
    out.append(("last_frame_whole", plant(P0 + F + BODY + 1, [(P0, 0, ()), (P0 + F, 0, ())]), None, [rec(P0, 0, 0, 1, 1), rec(P0 + F, 0, 0, 1, 1)]))
    # p + 813 = n: it is not, and is not emitted -- but its sync word still supports the frame in front of it
    out.append(("last_frame_short", plant(P0 + F + BODY, [(P0, 0, ()), (P0 + F, 0, ())]), None, [rec(P0, 0, 0, 1, 1)]))
    # two heads 828 bits apart, equal keys: the one in front stands (X1 = P0 + F against Y0 = P0 + F + 828)
    n6 = P0 + 3 * F + BODY + 40
    x1, y0 = P0 + F, P0 + F + 828
    out.append(("apart_828_position", plant(n6, [(P0, 0, ()), (x1, 0, ()), (y0, 0, ()), (y0 + F, 0, ())]), None,
                [rec(P0, 0, 0, 1, 1), rec(x1, 0, 0, 1, 1), rec(y0 + F, 0, 0, 1, 1)]))
    # ... by key: X1 with one wrong bit loses to Y0
    out.append(("apart_828_key", plant(n6, [(P0, 0, ()), (x1, 0, (5,)), (y0, 0, ()), (y0 + F, 0, ())]), None,
                [rec(P0, 0, 0, 1, 1), rec(y0, 0, 0, 1, 1), rec(y0 + F, 0, 0, 1, 1)]))
    # 829 apart: both stand, their frames overlap by three bits
    out.append(("apart_829", plant(n6, [(P0, 0, ()), (x1, 0, ()), (y0 + 1, 0, ()), (y0 + 1 + F, 0, ())]), None,
                [rec(P0, 0, 0, 1, 1), rec(x1, 0, 0, 1, 1), rec(y0 + 1, 0, 0, 1, 1), rec(y0 + 1 + F, 0, 0, 1, 1)]))
    # a chain A > B > C: A (u = 2) beats B = A + 500 (u = 1), B beats C = A + 1000 (equal keys, B in front), A does not reach C.  C is
    # dropped although B is: the rule judges against heads, not against what was emitted.  B's partner B - F loses to A - F and A,
    # C's partner C + F stands
    a, b, c = A3, A3 + 500, A3 + 1000
    out.append(("chain_A_B_C", plant(c + F + BODY + 40, [(a - 2 * F, 0, ()), (a - F, 0, ()), (a, 0, ()), (b - F, 0, ()), (b, 0, ()), (c, 0, ()), (c + F, 0, ())]),
                None, [rec(a - 2 * F, 0, 0, 2, 1), rec(a - F, 0, 0, 2, 1), rec(a, 0, 0, 2, 1), rec(c + F, 0, 0, 1, 1)]))
    # E = 0 through the zero_mask form: one wrong bit is no candidate any more
    out.append(("E0_exact", plant(n5, [(P0, 0, ()), (P0 + F, 0, (7,)), (P0 + 2 * F, 0, ())]), (0, 2, 3), [rec(P0, 0, 0, 1, 1), rec(P0 + 2 * F, 0, 0, 1, 1)]))
    # E = 3, W = 1 (G can only be 2): slots 0 (three wrong bits) and 2 do not see each other, but the empty slot between them sees both
    # -- a flywheel head on 19 zero bits: 10 of them wrong (the ones of S)
    out.append(("E3_W1", plant(n5, [(P0, 0, (1, 2, 3)), (P0 + 2 * F, 0, ())]), (3, 1, 2), [rec(P0 + F, 0, 10, 2, 0)]))
    # E = 3, W = 2: they do, and with G = 3 the slot between is none
    out.append(("E3_W2", plant(n5, [(P0, 0, (1, 2, 3)), (P0 + 2 * F, 0, ())]), (3, 2, 3), [rec(P0, 0, 3, 1, 1), rec(P0 + 2 * F, 0, 0, 1, 1)]))
    # G = 2: the empty slot between two sync words is a flywheel head; the slots on the outside see one neighbour only
    out.append(("G2", plant(n5, [(P0 + F, 0, ()), (P0 + 3 * F, 0, ())]), (2, 2, 2),
                [rec(P0 + F, 0, 0, 1, 1), rec(P0 + 2 * F, 0, 10, 2, 0), rec(P0 + 3 * F, 0, 0, 1, 1)]))
    # W = 8: a neighbour eight slots away counts
    n9 = P0 + 8 * F + BODY + 40
    out.append(("W8", plant(n9, [(P0, 0, ()), (P0 + 8 * F, 0, ())]), (2, 8, 16), [rec(P0, 0, 0, 1, 1), rec(P0 + 8 * F, 0, 0, 1, 1)]))
    out.append(("W7", plant(n9, [(P0, 0, ()), (P0 + 8 * F, 0, ())]), (2, 7, 14), []))
    # nothing at all
    out.append(("empty", b"", None, []))
    out.append(("n18", b"1" * 18, None, []))
    out.append(("n831", plant(831, [(18, 0, ())]), None, []))
    return out


def random_strings(count: int = 200, seed: int = 20):
    """count strings of 2 000 .. 6 000 random bits with planted sync words: chains at F (sometimes F +- 1, or anywhere), 0 .. 4 wrong
    bits each, both polarities"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(2000, 6001))
        b = rng.integers(0, 2, n).astype(np.uint8)
        for _chain in range(int(rng.integers(1, 4))):
            p, inv = int(rng.integers(0, F)), int(rng.integers(0, 2))
            while p < n:
                if rng.random() < 0.85:
                    w = [int(c) ^ inv for c in S]
                    for k in rng.choice(19, size=int(rng.integers(0, 5)), replace=False):
                        w[k] ^= 1
                    for j in range(19):
                        if 0 <= p - 18 + j < n:
                            b[p - 18 + j] = w[j]
                step = float(rng.random())
                p += F if step < 0.8 else F + int(rng.integers(-1, 2)) if step < 0.9 else int(rng.integers(20, 2 * F))
        out.append(bytes(b + ord("0")))
    return out


def seam_strings(T: int):
    """(name, bits): what a wrong kernel gets wrong at the seams of tiles of T bits -- none longer than about 6 T"""
    out = []
    n = 4 * T
    # sync words that straddle the seam at 2 T at every one of the 19 offsets (p = 2 T - 1 .. 2 T + 17: 0 .. 18 bits behind the seam),
    # each with a partner one frame on
    for k in range(19):
        p = 2 * T - 1 + k
        out.append((f"straddle_{k}", plant(n, [(p, k & 1, ()), (p + F, k & 1, (k,))], seed=k + 1)))
    # a flywheel head whose four neighbours lie in four other tiles (W = 2: F = 832 < T, so the slots are spread with a larger window --
    # the neighbours at +-4 F and +-8 F of a head in tile 3; every slot between is empty), and the plain version at W = 2 across one seam
    h = 3 * T + 2000
    assert len({(h + k * F) // T for k in (-8, -4, 0, 4, 8)}) == 5
    out.append(("flywheel_four_tiles", plant(h + 8 * F + BODY + 5, [(h - 8 * F, 0, ()), (h - 4 * F, 0, ()), (h + 4 * F, 0, ()), (h + 8 * F, 0, ())], seed=3),
                (2, 8, 4)))
    out.append(("flywheel_across_seam", plant(n, [(2 * T - F - 3, 1, ()), (2 * T - 2 * F - 3, 1, ()), (2 * T + F - 3, 1, ())], seed=4)))
    # a conflict pair split by a seam: 828 and 829 apart, either side winning
    for d, flips in ((828, ()), (828, (4,)), (829, ())):
        g = 2 * T - 400
        out.append((f"conflict_{d}_{len(flips)}", plant(n, [(g - F, 0, ()), (g, 0, flips), (g + d, 0, ()), (g + d + F, 0, ())], seed=5)))
    # strings of exactly T, T +- 1 and 13 * 64 * k +- 1 bits, a chain running to the very end
    for m in (T, T - 1, T + 1, 2 * T, 2 * T + 1, F * 5 - 1, F * 5, F * 5 + 1, F * 10 - 1, F * 10 + 1):
        last = m - 1 - BODY
        words = [(last - k * F, 0, ()) for k in range(0, 1 + (last - 18) // F)]
        out.append((f"length_{m}", plant(m, words, seed=6)))
        out.append((f"length_{m}_short", plant(m, [(p + 1, 0, ()) for p, _, _ in words if p + 1 < m], seed=7)))
    return [(t[0], t[1], t[2] if len(t) > 2 else None) for t in out]
