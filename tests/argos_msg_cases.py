"""Bit strings for the ARGOS message tests (no fixtures here: a plain module beside real_captures.py), shared by
tests/test_argos_messages.py (the host restatement against the Python model) and tests/test_gpu_argos_messages.py (the kernels against
the host restatement).  Strings are bytes of '0'/'1'; a case is (name, string, min_run)."""
import numpy as np

SYNC = "000101111"                                       # the frame sync 00010111 and the initialisation bit
CODES = ("0000", "0011", "0101", "0110", "1001", "1010", "1100", "1111")          # N = 1 .. 8
BAD_CODES = tuple(f"{v:04b}" for v in range(16) if f"{v:04b}" not in CODES)


def flip(s: str) -> str:
    return s.translate(str.maketrans("01", "10"))


def bits_of(value: int, width: int) -> str:
    return format(value, f"0{width}b")


def body(n: int, ident: int, data: bytes) -> str:
    assert len(data) == 4 * n and 0 <= ident < (1 << 20)
    return bits_of(ident, 20) + "".join(bits_of(b, 8) for b in data)


def message(n: int, ident: int, data: bytes, inverted: int = 0, run: str = "1" * 15, code: str | None = None) -> str:
    """the RAW bits `run` (as they are, whatever the polarity), then sync, length code and body in the message's polarity"""
    m = SYNC + (CODES[n - 1] if code is None else code) + body(n, ident, data)
    return run + (flip(m) if inverted else m)


def data_for(n: int, salt: int) -> bytes:
    return bytes((37 * salt + 11 * k + 3) & 0xFF for k in range(4 * n))


def crafted():
    """(name, string, min_run) of every crafted case of the issue"""
    cases = []
    noise = "0110100110010110"                           # no sync, no long run
    for n in range(1, 9):
        for inv in (0, 1):
            for rv in "01":
                cases.append((f"len{n}-inv{inv}-run{rv}", noise + message(n, 0x12345 + n, data_for(n, n), inv, rv * 15) + noise, 6))
    for code in BAD_CODES:
        for inv in (0, 1):
            cases.append((f"badcode{code}-inv{inv}", noise + message(1, 0xABCDE, data_for(1, 9), inv, "1" * 15, code=code) + noise, 6))
    for k in (0, 1, 6, 15):
        for inv in (0, 1):
            for rv in "01":
                other = flip(rv)
                # exactly K equal bits behind a different one; K - 1 equal bits (no head unless K = 0); the head at e = 12 + K and at 12 + K - 1
                cases.append((f"K{k}-exact-inv{inv}-run{rv}", noise + other + message(2, 0x0F0F0, data_for(2, k), inv, rv * k) + noise, k))
                if k:
                    cases.append((f"K{k}-short-inv{inv}-run{rv}", noise + other + message(2, 0x0F0F0, data_for(2, k), inv, rv * (k - 1)) + noise, k))
                cases.append((f"K{k}-first-inv{inv}-run{rv}", message(3, 0x54321, data_for(3, k), inv, rv * k) + noise, k))
                if k:
                    cases.append((f"K{k}-before-first-inv{inv}-run{rv}", message(3, 0x54321, data_for(3, k), inv, rv * (k - 1)) + noise, k))
    for n in (1, 3, 8):
        whole = message(n, 0x77777, data_for(n, 20 + n), n & 1, "0" * 15)
        head = 15 + 13
        for cut in (0, 19, 20, 21, 20 + 32 * n - 1, 20 + 32 * n):
            cases.append((f"cut{cut}-len{n}", noise + whole[: head + cut], 6))
    # two messages back to back: the second's run is the end of the first's data (K = 6), or none is asked for (K = 0)
    first = message(1, 0x11111, bytes([1, 2, 3, 0xC0]), 0, "1" * 15)
    cases.append(("back-to-back-K6", noise + first + message(2, 0x22222, data_for(2, 5), 1, "") + noise, 6))
    cases.append(("back-to-back-K0", noise + message(1, 0x11111, data_for(1, 6), 1, "") + message(2, 0x22222, data_for(2, 7), 0, "") + noise, 0))
    # a head inside an accepted body (its run, sync and code are data bits), followed by one just behind the body
    inner = "111111" + SYNC + "0011"                     # 19 bits of the 32 N data bits
    for inv_outer in (0, 1):
        for k in (0, 6):
            payload = inner + "0" * (64 - len(inner) - 6) + "000000"
            data = bytes(int(payload[i: i + 8], 2) for i in range(0, 64, 8))
            outer = message(2, 0x33333, data, inv_outer, "1" * 15)
            behind = message(1, 0x44444, data_for(1, 8), 0, "")
            cases.append((f"inside-inv{inv_outer}-K{k}", noise + outer + behind + noise, k))
            # the same head when the body it lay in is absent: accepted
            cases.append((f"inside-alone-inv{inv_outer}-K{k}", noise + (flip(payload) if inv_outer else payload) + noise * 4, k))
    cases.append(("empty", "", 6))
    cases.append(("short", "0001011110000", 0))
    cases.append(("twelve", "000101111000", 0))
    out = [(name, s.encode(), k) for name, s, k in cases]
    # bytes other than '0' / '1': every one of them is a one
    base = (noise + message(2, 0xFEDCB, data_for(2, 3), 1, "1" * 15) + noise).encode()
    for name, one in (("x", b"x"), ("nul", b"\x00"), ("ff", b"\xff"), ("one", b"\x01")):
        out.append((f"other-bytes-{name}", base.replace(b"1", one), 6))
    mixed = bytearray(base)
    for i in range(len(mixed)):
        if mixed[i] == ord("1"):
            mixed[i] = (i * 37 + 2) & 0xFF if ((i * 37 + 2) & 0xFF) != ord("0") else 7
    out.append(("other-bytes-mixed", bytes(mixed), 6))
    return out


def random_bits(n: int = 20000, seed: int = 7) -> bytes:
    return (np.random.RandomState(seed).randint(0, 2, n).astype(np.uint8) + ord("0")).tobytes()


def at_seams(tile: int, limit: int = 9000):
    """(name, string, min_run): for every k with tile * k < limit a head whose e is tile * k - 1, tile * k and tile * k + 1; a sync word
    (with its length code, 13 bits) straddling the first seam at each of its 13 positions; a body that spans three tiles; a string of 3
    tiles + 1 bit that ends in a head."""
    cases = []
    filler = "01" * (limit + 4 * tile)

    def place(e: int, msg: str, lead: int, length: int) -> str:
        """`msg` = run + sync + code + body with `lead` run bits, placed so that the length code ends at bit e, in `length` bits of filler"""
        start = e - (lead + 12)
        assert start >= 0
        s = filler[:start] + msg
        return (s + filler[: max(0, length - len(s))])[:max(length, len(s))]

    k = 1
    while tile * k < limit:
        for d in (-1, 0, 1):
            for inv in (0, 1):
                m = message(2, 0x5A5A5, data_for(2, k + d + 1), inv, "1" * 15)
                cases.append((f"seam{k}{d:+d}-inv{inv}", place(tile * k + d, m, 15, tile * k + 200), 6))
        k += 1
    for pos in range(13):                                # bit `pos` of the 13 is the first bit of the second tile
        m = message(1, 0x13579, data_for(1, pos), pos & 1, "0" * 15)
        cases.append((f"straddle{pos}", place(tile + 12 - pos, m, 15, tile + 300), 6))
    # bodies over seams.  The longest body is 276 bits: one spans three tiles only if the tile is shorter than that; with a longer
    # tile the three tiles hold a body over each of their two seams instead
    m = message(8, 0xCAFE5, data_for(8, 77), 1, "1" * 15)
    cases.append(("body-over-seam", place(tile - 3, m, 15, 3 * tile), 6))
    if tile < 276:
        cases.append(("three-tiles", place(tile - 3, m, 15, 4 * tile), 6))
    else:
        s = filler[: 3 * tile]
        for e, m in ((tile - 100, message(8, 0x0BEEF, data_for(8, 5), 0, "1" * 15)), (2 * tile - 5, message(8, 0x1BEEF, data_for(8, 6), 1, "0" * 15))):
            s = s[: e - 27] + m + s[e - 27 + len(m):]
        assert len(s) == 3 * tile
        cases.append(("three-tiles", s, 6))
    last = message(1, 0x24680, data_for(1, 1), 0, "1" * 15)[:28]          # run, sync and code: the head ends at the string's last bit
    s = filler[: 3 * tile + 1 - 28] + last
    assert len(s) == 3 * tile + 1
    cases.append(("three-tiles-plus-one", s, 6))
    return [(name, s.encode(), k) for name, s, k in cases]
