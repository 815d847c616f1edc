"""The ARGOS messages' second rule, PDT_ARGOS_RULE_BEST, on the GPU: k_argos_heads and k_argos_pick against the host
restatement, byte for byte, on every string of the CPU tests, with stray bits, runs and whole clusters at the tile seams and at the
pick kernel's tile-group boundary, past the cluster cap and past the accepted list; the chain on the real recording with everything
else a context holds left as it was; the per-burst windows of the wideband capture at which rule 0 loses half the messages; -R on the
command line; error codes."""
import os
import subprocess

import numpy as np
import pytest

import argos_best_cases as bc
import real_captures as rc
import test_argos_messages as cpu
from conftest import ROOT
from test_gpu_argos_messages import held, same_content
from test_windows import D, FS, IN_RATE, to_cu8

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bin")
PAIR, SECONDS = (210, 214), 6.0


@pytest.fixture(scope="module")
def argos(pdt):
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as d:
        yield d


@pytest.fixture(scope="module")
def pair(pdt):
    return bc.kind2_pair(pdt, PAIR, SECONDS)


@pytest.fixture(scope="module")
def host_pipeline(pdt, orc, pair):
    """the host pipeline's windows and, per rule, what each window decodes to"""
    x, params = pair
    win, bits = bc.host_window_bits(pdt, orc, x)
    return win, {rule: [bc.decoded(pdt.host_argos_messages(b, rule=rule)) for b in bits] for rule in (0, 1)}


def test_stage_equals_host_on_every_cpu_case(pdt, argos):
    cases = bc.crafted_best() + bc.existing(pdt.argos_msg_tile())
    found = slips = 0
    for name, bits, k in cases:
        want = pdt.host_argos_messages(bits, min_run=k, rule=1)
        found += len(want)
        slips += int(pdt.argos_slip(want).sum())
        assert argos.stage_argos_messages(bits, min_run=k, rule=1).tobytes() == want.tobytes(), name
    assert found > 600 and slips > 20
    bits = cases[0][1]
    assert argos.stage_argos_messages(bits, rule=1).tobytes() == pdt.host_argos_messages(bits, min_run=6, rule=1).tobytes()      # the default run


def test_stage_at_tile_seams_and_the_tile_group_boundary(pdt, argos):
    tile = pdt.argos_msg_tile()
    cases = bc.best_seams(tile)
    assert len(cases) == 9 * ((9000 - 1) // tile + 1) and max(len(bits) for _, bits, _ in cases) < 300000
    for name, bits, k in cases:
        want = pdt.host_argos_messages(bits, min_run=k, rule=1)
        # the stray bit's head is a slip with the whole run; of a cluster the inner head alone is left
        if name.endswith("-stray"):
            assert [(r["id"], r["reserved_"]) for r in want] == [(0x5A5A5, 15 | 1 << 8)], name
        else:
            assert [(r["id"], r["reserved_"]) for r in want] == [(0x0BBBB, 15)], name
        assert argos.stage_argos_messages(bits, min_run=k, rule=1).tobytes() == want.tobytes(), name
    at = sorted({int(pdt.host_argos_messages(bits, rule=1)[0]["bit_index"]) for name, bits, _ in cases if name.endswith(("-stray", "-inner"))})
    assert at == sorted(s + d for s in [k * tile for k in range(1, (9000 - 1) // tile + 1)] + [64 * tile] for d in (-1, 0, 1))


def test_stage_past_the_cluster_cap_and_past_the_list(pdt, argos):
    by = {name: (bits, k) for name, bits, k in bc.crafted_best()}
    for name in ("capped-cluster", "capped-cluster-decides"):
        bits, k = by[name]
        want = pdt.host_argos_messages(bits, min_run=k, rule=1)
        assert len(want) > 50
        assert argos.stage_argos_messages(bits, min_run=k, rule=1).tobytes() == want.tobytes(), name
    bits = bc.long_random()
    want, n = pdt.host_argos_messages(bits, min_run=0, rule=1, with_count=True)
    assert n == len(want) > 256
    got, found = argos.stage_argos_messages(bits, min_run=0, rule=1, with_count=True)
    assert found == n and got.tobytes() == want.tobytes()
    # a cap smaller than what is found: the count is still reported
    for cap in (0, 5, 256, 257):
        got, found = argos.stage_argos_messages(bits, min_run=0, rule=1, cap=cap, with_count=True)
        assert found == n and got.tobytes() == want[:cap].tobytes(), cap
    for k in (1, 6, 15):
        assert argos.stage_argos_messages(bits, min_run=k, rule=1).tobytes() == pdt.host_argos_messages(bits, min_run=k, rule=1).tobytes(), k
    # rule 0 on the same context afterwards: its own bytes, reserved_ 0
    got = argos.stage_argos_messages(bits, min_run=0, rule=0)
    assert got.tobytes() == pdt.host_argos_messages(bits, min_run=0).tobytes() and not got["reserved_"].any()


@pytest.mark.parametrize("cut,bit_index,run_value", ((1000, 87, 1), (3000, 62, 0)))
def test_chain_on_the_real_recording(pdt, argos, cut, bit_index, run_value):
    rate, iq = rc.capture("packet")
    argos.demod(iq[cut:])
    before = held(pdt, argos)
    today = argos.argos_messages()
    m = argos.argos_messages(rule=pdt.ARGOS_RULE_BEST)
    assert held(pdt, argos) == before
    cpu.the_real_message(m, bit_index, run_value)
    assert (pdt.argos_run_len(m)[0], pdt.argos_slip(m)[0]) == (15, 0)
    assert same_content(m, pdt.host_argos_messages(argos.stage(pdt.ST_BITS), rule=1))
    for f in ("time", "time_src"):
        assert m[0][f] == today[0][f]
    src = int(argos.stage(pdt.ST_SYMIDX)[argos.stage(pdt.ST_BITSYM)[bit_index]])
    assert m[0]["time_src"] == src and m[0]["time"] == pdt.time_axis(pdt.MODE_ARGOS, rate, src + 1)
    assert pdt.format_argos_messages(m).endswith(b"i 1 01D81 00 55 AA FF\n")
    # rule 0 afterwards gives today's bytes
    assert argos.argos_messages(rule=0).tobytes() == today.tobytes() == argos.argos_messages().tobytes() and not today["reserved_"].any()
    assert held(pdt, argos) == before


def test_wideband_windows(pdt, pair, host_pipeline):
    """seeds (210, 214), 6 s: under rule 1 every window gives the message sent for its burst and nothing else, as the host pipeline
    does; under rule 0 the same contexts give the host pipeline's 4 right windows; one batch call equals eight single calls"""
    x, params = pair
    host_win, host = host_pipeline
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x), IN_RATE, len(x))
        assert len(windows) == 8 and [w.first_frame for w in windows] == [w.first_frame for w in host_win]
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS, profile=(i == 0)).set_channel(D, 0.0) for i in range(len(windows))]
        try:
            pdt.demod_windows(ds, x, 0, 0, windows)
            best = pdt.argos_messages_batch(ds, rule=pdt.ARGOS_RULE_BEST)
            times = ds[0].kernel_times()
            assert times["k_argos_heads"][0] == 1 and times["k_argos_pick"][0] == 1
            want = [[bc.sent_for_window(pdt, params, w)] for w in windows]
            each = [bc.decoded(m) for m in best]
            print("rule 1, windows with exactly their message:", sum(e == w for e, w in zip(each, want)), "of", len(windows))
            assert each == want and each == host[1] and all(len(m) == 1 for m in best)
            assert {e[0][0] for e in each} == set(range(1, 9))
            first = pdt.argos_messages_batch(ds, rule=pdt.ARGOS_RULE_FIRST)
            each0 = [bc.decoded(m) for m in first]
            print("rule 0, windows with exactly their message:", sum(e == w for e, w in zip(each0, want)), "of", len(windows))
            assert each0 == host[0] and sum(e == w for e, w in zip(each0, want)) == 4
            assert [m.tobytes() for m in first] == [m.tobytes() for m in pdt.argos_messages_batch(ds)]
            assert [m.tobytes() for m in best] == [d.argos_messages(rule=1).tobytes() for d in ds]
            for d, m in zip(ds, best):
                assert same_content(m, pdt.host_argos_messages(d.stage(pdt.ST_BITS), rule=1))
        finally:
            for d in ds:
                d.close()


def test_command_line(pdt, pair, tmp_path):
    exe = os.path.join(BIN, "demodARGOS")
    x, params = pair
    x8 = to_cu8(x)
    cu8 = str(tmp_path / "capture.cu8")
    x8.tofile(cu8)
    base = [exe, "-x", str(D), "-s", str(IN_RATE // 1000), "-t", "each"]
    text = {}
    for name, extra in (("best", ["-R", "best"]), ("first", ["-R", "first"]), ("none", [])):
        out, pk = str(tmp_path / f"{name}.txt"), str(tmp_path / f"{name}.packets")
        r = subprocess.run(base + ["-A", out, "-o", pk] + extra + [cu8], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        text[name] = open(out, "rb").read()
    with pdt.Demodulator(pdt.MODE_ARGOS, FS) as holder:
        holder.set_channel(D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x8, max_s=5.0), IN_RATE, len(x8))
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, FS).set_channel(D, 0.0) for _ in windows]
        try:
            holder.demod_windows_held(ds, windows)
            parts = {rule: pdt.argos_messages_batch(ds, rule=rule) for rule in (0, 1)}
            for rule in parts:
                for part, w in zip(parts[rule], windows):
                    part["time"] += w.first_frame / IN_RATE
        finally:
            for d in ds:
                d.close()
    # without -R it writes what it writes today: rule 0's text; with -R best the eight lines, one per window, of the messages sent
    assert text["none"] == text["first"] == pdt.format_argos_messages(np.concatenate(parts[0]))
    assert text["best"] == pdt.format_argos_messages(np.concatenate(parts[1])) and text["best"].count(b"\n") == 8
    assert len(windows) == 8 and [bc.decoded(m) for m in parts[1]] == [[bc.sent_for_window(pdt, params, w)] for w in windows]
    assert text["best"] != text["none"]
    # the one-shot route, and an unknown rule
    out = str(tmp_path / "one.txt")
    r = subprocess.run([exe, "-A", out, "-R", "best", "-o", str(tmp_path / "one.packets"), rc.PACKET_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(out, "rb").read() == b""               # (uncut, the recording's message is not found under either rule)
    r = subprocess.run([exe, "-A", out + "x", "-R", "last", rc.PACKET_WAV], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "-R first or -R best" in r.stdout and not os.path.exists(out + "x")


def test_rule_2_is_refused_and_the_context_untouched(pdt, argos):
    rate, iq = rc.capture("packet")
    argos.demod(iq[1000:])
    before = held(pdt, argos)
    for bad in (2, -1):
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.argos_messages(rule=bad)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            argos.stage_argos_messages(b"0101", rule=bad)
        with pytest.raises(pdt.PdtError, match=r"\(-1\)"):
            pdt.argos_messages_batch([argos], rule=bad)
    assert held(pdt, argos) == before
    cpu.the_real_message(argos.argos_messages(rule=1), 87, 1)
    cpu.the_real_message(argos.argos_messages(), 87, 1)
