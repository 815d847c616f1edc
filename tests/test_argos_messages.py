"""The ARGOS messages in a bit stream, without a GPU: pdt_host_argos_messages against a Python model written here from
the rule's text (include/pdt.h), field for field, on crafted strings and on random bits; the real recording, whose message the
reference's framing loses (inverted, ID 01D81, data 00 55 AA FF); the golden synthetic capture upright and with Q negated; the synthetic
messages of every length (kind 2); the text.  The oracle's chain supplies the bits."""
import ctypes as C
import os

import numpy as np
import pytest

import real_captures as rc
from argos_msg_cases import at_seams, crafted, random_bits
from test_windows import ARGOS_RANGE, D, FS, IN_RATE, OFFSETS, PERIOD_S, RESIDUAL

LENGTHS = {"0000": 1, "0011": 2, "0101": 3, "0110": 4, "1001": 5, "1010": 6, "1100": 7, "1111": 8}
KIND2_SEED = 99                  # the oracle's chain decodes all nine bursts of 13 s at this seed (test_kind2_every_length)
WB_SEEDS, WB_SECONDS = (206, 210), 6.0     # ... and every window of the two wideband platforms at these (test_kind2_wideband_host_pipeline)


def model(bits: bytes, k: int = 6):
    """The rule, from its text: a list of dicts in ascending e."""
    b = [0 if v == ord("0") else 1 for v in bits]
    n = len(b)
    raw = "".join(map(str, b))
    comp = raw.translate(str.maketrans("01", "10"))
    out, last_end = [], -1
    for e in range(12 + k, n):
        for p, c in ((0, raw), (1, comp)):
            if c[e - 12: e - 3] != "000101111" or c[e - 3: e + 1] not in LENGTHS:
                continue
            if k and len(set(raw[e - 12 - k: e - 12])) != 1:
                continue
            if e - 12 <= last_end:
                continue                                  # begins inside the body accepted before it: no trace
            blocks = LENGTHS[c[e - 3: e + 1]]
            want = 20 + 32 * blocks
            have = min(want, n - (e + 1))
            bodybits = c[e + 1: e + 1 + have] + "0" * (want - have)
            data = bytes(int(bodybits[20 + 8 * i: 28 + 8 * i], 2) for i in range(4 * blocks))
            out.append(dict(bit_index=e, time_src=e, time=float(e), id=int(bodybits[:20], 2), blocks=blocks, inverted=p,
                            complete=int(have == want), run_value=int(c[e - 13]) if k else 0, data_bits=max(0, have - 20),
                            data=data + bytes(32 - len(data))))
            last_end = e + want
    return out


def same(records, want) -> bool:
    if len(records) != len(want):
        return False
    for r, w in zip(records, want):
        for f in ("bit_index", "time_src", "time", "id", "blocks", "inverted", "complete", "run_value", "data_bits"):
            if r[f] != w[f]:
                return False
        if bytes(r["data"]) != w["data"] or r["reserved_"] != 0:
            return False
    return True


def fmt_py(records) -> bytes:
    out = []
    for r in records:
        if r["complete"]:
            out.append(b"%.5f%s %d %05X" % (r["time"], b"i" if r["inverted"] else b"", r["blocks"], r["id"])
                       + b"".join(b" %02X" % v for v in bytes(r["data"])[: 4 * r["blocks"]]) + b"\n")
    return b"".join(out)


CRAFTED = crafted()


def test_the_cases_cover_what_they_are_meant_to():
    """the crafted strings do hold (or do not hold) what their names say, by the model"""
    by = {name: model(s, k) for name, s, k in CRAFTED}
    for n in range(1, 9):
        for inv in (0, 1):
            for rv in (0, 1):
                m = by[f"len{n}-inv{inv}-run{rv}"]
                assert len(m) == 1 and (m[0]["blocks"], m[0]["inverted"], m[0]["run_value"], m[0]["complete"]) == (n, inv, rv ^ inv, 1)
    none = [name for name in by if name.startswith(("badcode", "empty", "twelve")) or "-short-" in name or "-before-first-" in name]
    # (any single bit is a run of one: "K1-short" holds a head, the bit in front of it is its run)
    assert all((len(by[name]) == 1) if name.startswith("K1-short") else by[name] == [] for name in none) and len(none) > 40
    for k in (0, 1, 6, 15):
        assert all(len(by[f"K{k}-exact-inv{i}-run{r}"]) == 1 for i in (0, 1) for r in "01")
        assert all([m["bit_index"] for m in by[f"K{k}-first-inv{i}-run{r}"]] == [12 + k] for i in (0, 1) for r in "01")
    for n in (1, 3, 8):
        got = {cut: by[f"cut{cut}-len{n}"] for cut in (0, 19, 20, 21, 20 + 32 * n - 1, 20 + 32 * n)}
        assert all(len(v) == 1 for v in got.values())
        assert [got[c][0]["data_bits"] for c in (0, 19, 20, 21, 20 + 32 * n - 1)] == [0, 0, 0, 1, 32 * n - 1]
        assert [got[c][0]["complete"] for c in (0, 21, 20 + 32 * n - 1, 20 + 32 * n)] == [0, 0, 0, 1]
    assert [m["id"] for m in by["back-to-back-K6"]] == [0x11111, 0x22222] and [m["id"] for m in by["back-to-back-K0"]] == [0x11111, 0x22222]
    for inv in (0, 1):
        for k in (0, 6):
            assert [m["id"] for m in by[f"inside-inv{inv}-K{k}"]] == [0x33333, 0x44444]
            assert len(by[f"inside-alone-inv{inv}-K{k}"]) == 1
    assert len(by["short"]) == 1 and by["short"][0]["bit_index"] == 12
    assert all(len(by[name]) == 1 and by[name][0]["id"] == 0xFEDCB for name in by if name.startswith("other-bytes"))


@pytest.mark.parametrize("name,bits,k", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_host_equals_model_on_crafted_strings(pdt, name, bits, k):
    assert same(pdt.host_argos_messages(bits, min_run=k), model(bits, k))


def test_host_equals_model_at_seams_and_on_random_bits(pdt):
    for name, bits, k in at_seams(pdt.argos_msg_tile()):
        want = model(bits, k)
        assert want, name
        assert same(pdt.host_argos_messages(bits, min_run=k), want), name
    bits = random_bits()
    counts = {}
    for k in (0, 1, 6, 15):
        want = model(bits, k)
        counts[k] = len(want)
        assert same(pdt.host_argos_messages(bits, min_run=k), want), k
    assert same(pdt.host_argos_messages(bits), model(bits, 6))            # the default is 6
    print("heads in 20 000 random bits by min_run:", counts)
    assert counts[0] > 10


def test_arguments_and_capacity(pdt):
    L = pdt.lib()
    bits = random_bits()
    want = model(bits, 0)
    got, found = pdt.host_argos_messages(bits, min_run=0, cap=5, with_count=True)
    assert found == len(want) > 5 and same(got, want[:5])
    got, found = pdt.host_argos_messages(bits, min_run=0, cap=0, with_count=True)
    assert found == len(want) and len(got) == 0
    a = np.frombuffer(bits, dtype=np.uint8)
    out, count = np.zeros(4, dtype=pdt.ARGOS_MSG_DTYPE), C.c_int(0)
    for bad in (-1, 16):
        cfg = pdt.ArgosCfg(min_run=bad)
        assert L.pdt_host_argos_messages(a.ctypes.data, a.size, C.byref(cfg), out.ctypes.data, 4, C.byref(count)) == -1
    assert L.pdt_host_argos_messages(a.ctypes.data, a.size, None, out.ctypes.data, -1, C.byref(count)) == -1
    assert L.pdt_host_argos_messages(a.ctypes.data, a.size, None, out.ctypes.data, 4, None) == -1
    # min_run 0 without its flag bit is the default, with it no run is asked for
    cfg = pdt.ArgosCfg(min_run=0)
    assert L.pdt_host_argos_messages(a.ctypes.data, a.size, C.byref(cfg), out.ctypes.data, 0, C.byref(count)) == 0
    assert count.value == len(model(bits, 6))
    cfg = pdt.ArgosCfg(min_run=0, zero_mask=pdt.ARGOS_ZERO_MIN_RUN)
    assert L.pdt_host_argos_messages(a.ctypes.data, a.size, C.byref(cfg), out.ctypes.data, 0, C.byref(count)) == 0
    assert count.value == len(want)
    assert C.sizeof(pdt.ArgosMsg) == 72 and C.sizeof(pdt.ArgosCfg) == 16 and pdt.argos_msg_tile() > 0


def the_real_message(m, bit_index, run_value):
    assert len(m) == 1
    r = m[0]
    assert (r["inverted"], r["blocks"], r["id"], r["complete"], r["data_bits"]) == (1, 1, 0x01D81, 1, 32)
    assert bytes(r["data"]) == bytes([0x00, 0x55, 0xAA, 0xFF]) + bytes(28)
    assert (r["bit_index"], r["run_value"]) == (bit_index, run_value)


@pytest.mark.parametrize("cut,bit_index,run_value", ((1000, 87, 1), (3000, 62, 0)))
def test_real_recording_cut(pdt, orc, cut, bit_index, run_value):
    rate, iq = rc.capture("packet")
    o = orc.Oracle(orc.ARGOS, rate, iq[cut:])
    assert len(o.frames()) == 0
    bits = o.stage(orc.ST_BITS)
    m = pdt.host_argos_messages(bits)
    assert same(m, model(bits.tobytes()))
    the_real_message(m, bit_index, run_value)
    assert pdt.format_argos_messages(m).endswith(b"i 1 01D81 00 55 AA FF\n")


def test_real_recording_uncut_and_through_the_down_converter(pdt, orc):
    rate, iq = rc.capture("packet")
    bits = rc.oracle("packet", rc.ARGOS).stage(orc.ST_BITS)
    assert len(pdt.host_argos_messages(bits)) == 0 and model(bits.tobytes()) == []
    y = pdt.host_ddc(rate, 2, -470.0, iq)
    y16 = np.clip(np.round(y.reshape(-1, 2) * 32768.0), -32768, 32767).astype(np.int16)
    o = orc.Oracle(orc.ARGOS, rate // 2, y16)
    m = pdt.host_argos_messages(o.stage(orc.ST_BITS))
    assert len(o.frames()) == 0
    the_real_message(m, m[0]["bit_index"] if len(m) else -1, m[0]["run_value"] if len(m) else -1)


def golden_synth(pdt):
    return pdt.synth_capture(1, 32000, 13.0, f0_hz=120.0, seed=99), pdt.synth_params(1, 32000, 120.0, 99)


def payload_id_data(pdt, p, burst):
    v = int.from_bytes(bytes(pdt.synth_argos_payload(p, burst)), "big") >> 4        # the first 52 of the 56 payload bits
    return v >> 32, (v & 0xFFFFFFFF).to_bytes(4, "big")


def test_golden_synthetic_upright_and_q_negated(pdt, orc):
    syn, p = golden_synth(pdt)
    o = orc.Oracle(orc.ARGOS, 32000, syn)
    bits, times, frames = o.stage(orc.ST_BITS), o.stage(orc.ST_BITT), o.frames()
    m = pdt.host_argos_messages(bits)
    assert len(frames) == 9 and same(m, model(bits.tobytes())) and len(m) == 9
    for b, (r, f) in enumerate(zip(m, frames)):
        assert r["bit_index"] == f.bit_index and times[r["bit_index"]] == f.time           # a frame's index and a frame's time
        assert (r["inverted"], r["blocks"], r["complete"]) == (0, 1, 1)
        assert (r["id"], bytes(r["data"][:4])) == payload_id_data(pdt, p, b)
    values = sorted(int(r["run_value"]) for r in m)
    assert values == [0] * 4 + [1] * 5                                                      # the run has either value
    neg = syn * np.array([1, -1], dtype=np.int16)
    o = orc.Oracle(orc.ARGOS, 32000, neg)
    nbits = o.stage(orc.ST_BITS)
    mi = pdt.host_argos_messages(nbits)
    assert len(o.frames()) == 0 and len(mi) == 9 and same(mi, model(nbits.tobytes()))
    for b, r in enumerate(mi):
        assert (r["inverted"], r["blocks"], r["complete"]) == (1, 1, 1)
        assert (r["id"], bytes(r["data"][:4])) == payload_id_data(pdt, p, b)


def test_realnoise_and_clip(pdt, orc):
    o = rc.oracle("realnoise", rc.ARGOS)
    m = pdt.host_argos_messages(o.stage(orc.ST_BITS))
    frames = o.frames()
    assert len(frames) == 8 and [int(r["bit_index"]) for r in m] == [f.bit_index for f in frames]
    assert all((r["inverted"], r["blocks"], r["complete"]) == (0, 1, 1) for r in m)
    assert len(pdt.host_argos_messages(rc.oracle("clip", rc.ARGOS).stage(orc.ST_BITS))) == 0


def test_synth_kind2_leaves_kinds_0_and_1_alone_and_tells_what_it_sent(pdt):
    for seed in (0, 5, 99):
        p = pdt.synth_params(2, 32000, 120.0, seed)
        seen = set()
        for b in range(8):
            blocks, ident, data = pdt.synth_argos_message(p, b)
            assert blocks == 1 + (b + seed) % 8 and len(data) == 4 * blocks and 0 <= ident < (1 << 20)
            seen.add(blocks)
        assert seen == set(range(1, 9))
    # the carrier of a burst is on for 160 ms + (48 + 32 N) bits at 400 bit/s, then off: noise only
    p = pdt.synth_params(2, 32000, 120.0, 3)
    p.noise_gain = 0
    x = np.zeros((48000, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, len(x), x.ctypes.data)
    on = np.flatnonzero(np.abs(x).sum(axis=1) > 0)
    n0 = pdt.synth_argos_message(p, 0)[0]
    assert on[0] == 0 and on[-1] == 5120 + (48 + 32 * n0) * 80 - 1


def decoded(pdt, m):
    return [(int(r["blocks"]), int(r["id"]), bytes(r["data"][: 4 * r["blocks"]])) for r in m if r["complete"]]


def test_kind2_every_length(pdt, orc):
    """13 s at 32 ksps through the oracle: the nine messages sent, all eight lengths among them, and nothing else"""
    p = pdt.synth_params(2, 32000, 120.0, KIND2_SEED)
    x = pdt.synth_capture(2, 32000, 13.0, f0_hz=120.0, seed=KIND2_SEED)
    bits = orc.Oracle(orc.ARGOS, 32000, x).stage(orc.ST_BITS)
    m = pdt.host_argos_messages(bits)
    assert same(m, model(bits.tobytes()))
    sent = [pdt.synth_argos_message(p, b) for b in range(9)]
    assert decoded(pdt, m) == [(n, i, bytes(d)) for n, i, d in sent] and len(m) == 9
    assert {n for n, _, _ in sent} == set(range(1, 9))
    assert all(r["inverted"] == 0 for r in m)


def kind2_platforms(pdt, secs: float = WB_SECONDS):
    """two platforms of kind 2 in one wideband capture, as test_windows.platforms builds its kind-1 pair"""
    n = int(round(secs * IN_RATE))
    total = np.zeros((n, 2), dtype=np.int32)
    params = []
    for off, seed in zip(OFFSETS, WB_SEEDS):
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


def test_kind2_wideband_host_pipeline(pdt, orc):
    """host_bursts -> burst_windows -> host_ddc of each slice -> the oracle: every window yields the message sent for its burst and
    nothing else, all eight lengths among them (seeds four apart: four bursts of each platform cover them).  This pins the seeds the
    GPU test (tests/test_gpu_argos_messages.py) uses.  They are chosen: at most seeds this pipeline loses windows -- over the 12 pairs
    (200, 204) .. (211, 215) it decodes 6, 7, 5, 6, 6, 5, 8, 8, 6, 7, 4, 6 of 8, and of the 20 windows of 15 s it loses 1 to 9 over 170 pairs -- to a
    false head in the stretch where the loop pulls in, or to a stray bit between a run of zeros and the sync; the
    oracle's portable-math mode decodes the same windows at these seeds."""
    x, params = kind2_platforms(pdt)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, rows=False)
    win = pdt.burst_windows(found, IN_RATE, len(x))
    assert len(win) == 8
    lengths = set()
    for w in win:
        y = pdt.host_ddc(IN_RATE, D, w.offset_hz, x[w.first_frame: w.first_frame + w.nframes])
        y16 = np.clip(np.round(y.reshape(-1, 2) * 32768.0), -32768, 32767).astype(np.int16)
        for math_mode in (orc.MATH_LIBM, orc.MATH_PORTABLE):
            got = decoded(pdt, pdt.host_argos_messages(orc.Oracle(orc.ARGOS, FS, y16, math_mode=math_mode).stage(orc.ST_BITS)))
            assert got == [sent_for_window(pdt, params, w)], (w, math_mode)
        lengths.add(got[0][0])
    assert lengths == set(range(1, 9))


def test_text(pdt):
    by = {name: s for name, s, k in CRAFTED}
    bits = b"".join(s for name, s in by.items() if name.startswith("len")) + by["cut21-len3"]           # (the last body is cut)
    m = pdt.host_argos_messages(bits)
    assert any(not r["complete"] for r in m) and sum(r["complete"] for r in m) > 20 and any(r["inverted"] for r in m)
    m["time"] = m["bit_index"] / 400.0 + 0.123456
    text = pdt.format_argos_messages(m)
    assert text == fmt_py(m) and text.count(b"\n") == sum(r["complete"] for r in m)
    assert pdt.format_argos_messages(m[:0]) == b"" and pdt.format_argos_messages(m[m["complete"] == 0]) == b""
    L = pdt.lib()
    r, w = os.pipe()
    try:
        n = C.c_uint64(0)
        small = m[:6]
        assert L.pdt_write_argos_messages(small.ctypes.data, len(small), w, C.byref(n)) == 0
        assert os.read(r, 1 << 16) == fmt_py(small) and n.value == len(fmt_py(small))
    finally:
        os.close(r)
        os.close(w)
    assert L.pdt_write_argos_messages(m.ctypes.data, len(m), -1, None) == -1
