"""The ARGOS messages in a bit stream, on the GPU: the kernels against the host restatement on every string of
tests/argos_msg_cases.py, heads at every tile seam included; the chain on the real recording (the message the reference's framing
loses) with everything else a context holds left as it was; the channel route; the synthetic captures upright, Q-negated and on real
noise, one message per frame; one batch call against five single ones; error codes; the synthetic messages of every length one-shot and
through per-burst windows of a wideband capture; and -A on the command line."""
import os
import subprocess

import numpy as np
import pytest

import real_captures as rc
import test_argos_messages as cpu
from argos_msg_cases import at_seams, crafted, random_bits
from conftest import ROOT
from test_windows import D, FS, IN_RATE, to_cu8

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
CONTENT = ("bit_index", "id", "blocks", "inverted", "complete", "run_value", "data_bits", "reserved_")


@pytest.fixture(scope="module")
def argos(pdt):
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as d:
        yield d


def same_content(a, b) -> bool:
    """every field but the time stamps"""
    return len(a) == len(b) and all((a[f] == b[f]).all() for f in CONTENT) and a["data"].tobytes() == b["data"].tobytes()


def test_stage_equals_host_on_crafted_and_random_strings(pdt, argos):
    for name, bits, k in crafted():
        assert argos.stage_argos_messages(bits, min_run=k).tobytes() == pdt.host_argos_messages(bits, min_run=k).tobytes(), name
    bits = random_bits()
    for k in (None, 0, 1, 6, 15):
        got = argos.stage_argos_messages(bits, min_run=k)
        assert got.tobytes() == pdt.host_argos_messages(bits, min_run=k).tobytes(), k
    assert len(argos.stage_argos_messages(bits, min_run=0)) > 10


def test_stage_at_tile_seams(pdt, argos):
    tile = pdt.argos_msg_tile()
    cases = at_seams(tile)
    assert len(cases) >= 6 * ((9000 - 1) // tile) + 13 + 3
    for name, bits, k in cases:
        want = pdt.host_argos_messages(bits, min_run=k)
        assert len(want) >= 1, name
        assert argos.stage_argos_messages(bits, min_run=k).tobytes() == want.tobytes(), name
    assert len(cases[-1][1]) == 3 * tile + 1 and pdt.host_argos_messages(cases[-1][1])[-1]["bit_index"] == 3 * tile


def test_stage_capacity_and_what_it_leaves_alone(pdt, argos):
    bits = random_bits()
    want = pdt.host_argos_messages(bits, min_run=0)
    got, found = argos.stage_argos_messages(bits, min_run=0, cap=5, with_count=True)
    assert found == len(want) > 5 and got.tobytes() == want[:5].tobytes()
    got, found = argos.stage_argos_messages(bits, min_run=0, cap=0, with_count=True)
    assert found == len(want) and len(got) == 0
    # the stage entry works beside a capture's results, not on them
    rate, iq = rc.capture("packet")
    argos.demod(iq[1000:])
    before = held(pdt, argos)
    argos.stage_argos_messages(bits)
    assert held(pdt, argos) == before
    cpu.the_real_message(argos.argos_messages(), 87, 1)


def held(pdt, d):
    """what a context holds after a whole-capture call: frames, text, statistics and the bytes of every stage"""
    stages = tuple(d.stage(st).tobytes() if d.stage_len(st) else b"" for st in range(pdt.ST_CHANNEL + 1))
    return d.frames_array().tobytes(), d.text(), bytes(d.stats()), stages


@pytest.mark.parametrize("cut,bit_index,run_value", ((1000, 87, 1), (3000, 62, 0)))
def test_chain_on_the_real_recording(pdt, argos, cut, bit_index, run_value):
    rate, iq = rc.capture("packet")
    argos.demod(iq[cut:])
    before = held(pdt, argos)
    m = argos.argos_messages()
    assert held(pdt, argos) == before
    assert len(argos.frames_array()) == 0
    cpu.the_real_message(m, bit_index, run_value)
    bits = argos.stage(pdt.ST_BITS)
    assert same_content(m, pdt.host_argos_messages(bits))
    # the time stamp is a frame's: the interpolated sample behind the bit, through the context's time axis
    src = int(argos.stage(pdt.ST_SYMIDX)[argos.stage(pdt.ST_BITSYM)[bit_index]])
    assert m[0]["time_src"] == src and m[0]["time"] == pdt.time_axis(pdt.MODE_ARGOS, rate, src + 1)
    assert pdt.format_argos_messages(m).endswith(b"i 1 01D81 00 55 AA FF\n")


def test_chain_uncut_and_channel_route(pdt, argos):
    rate, iq = rc.capture("packet")
    argos.demod(iq)
    assert len(argos.argos_messages()) == 0
    with pdt.Demodulator(pdt.MODE_ARGOS, rate // 2) as d:
        d.set_channel(2, -470.0).demod_channel(iq)
        m = d.argos_messages()
        assert len(d.frames_array()) == 0
        cpu.the_real_message(m, m[0]["bit_index"] if len(m) else -1, m[0]["run_value"] if len(m) else -1)
        assert same_content(m, pdt.host_argos_messages(d.stage(pdt.ST_BITS)))


def test_synthetic_captures_one_message_per_frame(pdt, argos):
    syn, p = cpu.golden_synth(pdt)
    argos.demod(syn)
    m, fr = argos.argos_messages(), argos.frames_array()
    assert len(m) == len(fr) == 9
    for f in ("bit_index", "time_src", "time"):
        assert (m[f] == fr[f]).all(), f
    assert all((r["inverted"], r["blocks"], r["complete"]) == (0, 1, 1) for r in m)
    assert [(int(r["id"]), bytes(r["data"][:4])) for r in m] == [cpu.payload_id_data(pdt, p, b) for b in range(9)]
    assert sorted(int(r["run_value"]) for r in m) == [0] * 4 + [1] * 5
    argos.demod(syn * np.array([1, -1], dtype=np.int16))
    mi = argos.argos_messages()
    assert len(argos.frames_array()) == 0 and len(mi) == 9 and all(r["inverted"] == 1 and r["complete"] == 1 for r in mi)
    assert [(int(r["id"]), bytes(r["data"][:4])) for r in mi] == [cpu.payload_id_data(pdt, p, b) for b in range(9)]
    argos.demod(rc.capture("realnoise")[1])
    m, fr = argos.argos_messages(), argos.frames_array()
    assert len(m) == len(fr) == 8
    for f in ("bit_index", "time_src", "time"):
        assert (m[f] == fr[f]).all(), f
    assert same_content(m, pdt.host_argos_messages(argos.stage(pdt.ST_BITS)))


def test_batch_equals_single_calls_in_one_launch(pdt):
    rate, iq = rc.capture("packet")
    syn, _ = cpu.golden_synth(pdt)
    inputs = [iq[1000:], iq[3000:], iq, rc.capture("realnoise")[1], syn * np.array([1, -1], dtype=np.int16)]
    ds = [pdt.Demodulator(pdt.MODE_ARGOS, rate, profile=(i == 0)) for i in range(len(inputs))]
    try:
        for d, x in zip(ds, inputs):
            d.demod(x)
        single = [d.argos_messages() for d in ds]
        assert [len(s) for s in single] == [1, 1, 0, 8, 9]
        for k in (None, 0):
            want = [d.argos_messages(min_run=k) for d in ds]
            got = pdt.argos_messages_batch(ds, min_run=k)
            assert [g.tobytes() for g in got] == [w.tobytes() for w in want], k
            times = ds[0].kernel_times()
            assert times["k_argos_msgs"][0] == 1 and times["k_argos_finish"][0] == 1
        small = pdt.argos_messages_batch(ds, cap=2)
        assert [len(s) for s in small] == [1, 1, 0, 2, 2] and small[4].tobytes() == single[4][:2].tobytes()
        assert pdt.argos_messages_batch([]) == []
    finally:
        for d in ds:
            d.close()


def test_error_codes(pdt, argos):
    rate, iq = rc.capture("packet")
    argos.demod(iq[1000:])
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        pdt.argos_messages_batch([argos, argos])                              # two contexts on the same pointer
    for bad in (-1, 16):
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.argos_messages(min_run=bad)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.stage_argos_messages(b"0101", min_run=bad)
    with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
        argos.argos_messages(cap=-1)
    cpu.the_real_message(argos.argos_messages(), 87, 1)                       # a refused call changed nothing
    with pdt.Demodulator(pdt.MODE_POES, 50000) as poes:
        poes.demod(rc.capture("clip")[1][:30000])
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            poes.argos_messages()
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.argos_messages_batch([argos, poes])
    with pdt.Demodulator(pdt.MODE_ARGOS, rate) as d:
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.argos_messages()                                                # nothing demodulated yet
        d.demod(iq[1000:])
        assert len(d.argos_messages()) == 1
        d.stream_begin()
        d.stream_push(iq[:4800])
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.argos_messages()                                                # an open stream
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            pdt.argos_messages_batch([argos, d])
        d.stream_end()
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.argos_messages()                                                # ... and an ended one
        d.demod(iq[1000:])
        assert len(d.argos_messages()) == 1
        d.bytesync(np.frombuffer(b"0101" * 50, dtype=np.uint8))
        with pytest.raises(pdt.PdtError, match=r"\(-6\)"):
            d.argos_messages()                                                # a stage-level call took the bit buffer


def test_kind2_one_shot(pdt, orc, argos):
    """at the seed the CPU test fixed: what was sent, and the model on the oracle's bits"""
    p = pdt.synth_params(2, 32000, 120.0, cpu.KIND2_SEED)
    x = pdt.synth_capture(2, 32000, 13.0, f0_hz=120.0, seed=cpu.KIND2_SEED)
    argos.demod(x)
    m = argos.argos_messages()
    sent = [pdt.synth_argos_message(p, b) for b in range(9)]
    assert cpu.decoded(pdt, m) == [(n, i, bytes(d)) for n, i, d in sent] and len(m) == 9
    want = cpu.model(orc.Oracle(orc.ARGOS, 32000, x).stage(orc.ST_BITS).tobytes())
    assert [(r["id"], r["blocks"], r["inverted"], r["complete"], bytes(r["data"])) for r in m] == \
           [(w["id"], w["blocks"], w["inverted"], w["complete"], w["data"]) for w in want]


@pytest.fixture(scope="module")
def kind2_pair(pdt):
    return cpu.kind2_platforms(pdt)


def test_kind2_wideband_windows(pdt, kind2_pair):
    """two platforms of kind 2 at 1.024 Msps, decimation 32: every window's message is the one sent for its burst"""
    x, params = kind2_pair
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x), IN_RATE, len(x))
        assert len(windows) == 8
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, 0.0) for _ in windows]
        try:
            pdt.demod_windows(ds, x, 0, 0, windows)
            got = pdt.argos_messages_batch(ds)
            each = [cpu.decoded(pdt, g) for g in got]
            want = [[cpu.sent_for_window(pdt, params, w)] for w in windows]
            print("windows with exactly their message:", sum(e == w for e, w in zip(each, want)), "of", len(windows))
            assert each == want
            assert {e[0][0] for e in each} == set(range(1, 9))
        finally:
            for d in ds:
                d.close()


def test_command_line(pdt, argos, kind2_pair, tmp_path):
    exe = os.path.join(BIN, "demodARGOS")
    rate, iq = rc.capture("packet")
    # the real recording, the carrier found by the survey: one line, the API's time, no packets file
    m_txt, out = str(tmp_path / "m.txt"), str(tmp_path / "packets.txt")
    r = subprocess.run([exe, "-x", "2", "-t", "auto", "-A", m_txt, "-o", out, rc.PACKET_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    text = open(m_txt, "rb").read()
    assert text.count(b"\n") == 1 and text.endswith(b"i 1 01D81 00 55 AA FF\n") and not os.path.exists(out)
    import re
    khz = re.findall(r"^Channel 0 at ([+-][0-9.]+) Khz \(found", r.stdout, flags=re.M)
    assert len(khz) == 1
    with pdt.Demodulator(pdt.MODE_ARGOS, rate // 2) as d:
        d.set_channel(2, float(khz[0]) * 1000.0).demod_channel(iq)
        assert pdt.format_argos_messages(d.argos_messages()) == text
    # -t each on the wideband capture: the batch call's text, times from the capture's start; the packets file is what it is without -A
    x, _ = kind2_pair
    x8 = to_cu8(x)
    cu8 = str(tmp_path / "capture.cu8")
    x8.tofile(cu8)
    base = [exe, "-x", str(D), "-s", str(IN_RATE // 1000), "-t", "each"]
    a_txt, pk, pk0 = str(tmp_path / "a.txt"), str(tmp_path / "pk.txt"), str(tmp_path / "pk0.txt")
    r = subprocess.run(base + ["-A", a_txt, "-o", pk, cu8], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    r0 = subprocess.run(base + ["-o", pk0, cu8], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and open(pk, "rb").read() == open(pk0, "rb").read()
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x8, max_s=5.0), IN_RATE, len(x8))
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, 0.0) for _ in windows]
        try:
            holder.demod_windows_held(ds, windows)
            parts = pdt.argos_messages_batch(ds)
            for part, w in zip(parts, windows):
                part["time"] += w.first_frame / IN_RATE
        finally:
            for d in ds:
                d.close()
    text = open(a_txt, "rb").read()
    assert text == pdt.format_argos_messages(np.concatenate(parts)) and text.count(b"\n") >= 4
    # routes that leave no bits: demodPOES, a pipe
    rp = subprocess.run([os.path.join(BIN, "demodPOES"), "-A", m_txt + "x", rc.CLIP_WAV], capture_output=True, text=True, timeout=300)
    assert rp.returncode == 1 and "-A needs demodARGOS" in rp.stdout and not os.path.exists(m_txt + "x")
    rl = subprocess.run([exe, "-l", "-A", m_txt + "x", "-"], input="", capture_output=True, text=True, timeout=300)
    assert rl.returncode == 1 and "-A needs demodARGOS" in rl.stdout and not os.path.exists(m_txt + "x")
