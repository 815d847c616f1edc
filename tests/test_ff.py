"""Feed-forward ARGOS bits without a GPU: pdt_host_ff_bits against a Python model written from the rule's text -- numpy
float32 with sequential sums, an exact fused multiply-add, an integer metric -- field for field and bit pattern for bit pattern on small
streams; pdt_host_ff_mix against a double rotation; the real recording, uncut, which the chain never locks on; bursts sent at a wrong bit
rate, which only the rate grid decodes; the per-burst windows of a wideband capture, every one of them right; error codes."""
import ctypes as C

import numpy as np
import pytest

import argos_best_cases as bc
import ff_cases as fc
import real_captures as rc


def check_against_model(pdt, fs, y, R, ppm=None, residual=0.0):
    got = pdt.host_ff_bits(fs, y, rate_steps=R, rate_step_ppm=ppm, residual_hz=residual)
    v = pdt.host_ff_mix(fs, residual, y)
    tau, r, P, M, bits, soft, index, table = fc.model(v, fs, R, 625.0 if ppm is None else ppm)
    s = got.sync
    assert (s["residual_hz"], s["tone_valid"], s["step"]) == (residual, 1, round(residual * 2 ** 32 / fs) % 2 ** 32)
    assert (int(s["tau"]), int(s["rate"]), int(s["period"]), int(s["metric"]), int(s["nbits"])) == (tau, r, P, M, len(bits))
    assert got.bits.tobytes() == bits.tobytes() and got.index.tobytes() == index.tobytes()
    assert got.soft.view(np.uint32).tobytes() == soft.view(np.uint32).tobytes()
    return got, table


@pytest.mark.parametrize("H", (4, 10, 40))
@pytest.mark.parametrize("R", (0, 2))
def test_host_equals_the_model_on_small_streams(pdt, H, R):
    fs = 800 * H
    ties = clamps = 0
    for name, y in fc.small_streams(H):
        got, table = check_against_model(pdt, fs, y, R)
        top = max(table.values())
        ties += sum(m == top for m in table.values()) > 1 and top > 0
        clamps += any(abs(d) >= 2.0 ** 20 for d in got.soft if np.isfinite(d))
        if name in ("zeros", "real-only", "noise-n0", "noise-n1"):
            assert (int(got.sync["tau"]), int(got.sync["rate"]), int(got.sync["metric"])) == (0, 0, 0), name
        if name == "noise-n0" or name == "noise-n1" or name == f"noise-n{2 * H - 1}":
            assert len(got.bits) == 0
        if name == f"noise-n{2 * H}":
            assert len(got.bits) == 1 and int(got.sync["tau"]) == 0
    assert ties >= 1 and clamps >= 1


def test_host_equals_the_model_with_a_wide_rate_grid_and_a_residual(pdt):
    """rate steps of 2 % move the half-bit boundaries within a few bits; a residual turns the stream first"""
    rng = np.random.default_rng(77)
    for H, n in ((4, 131), (10, 173)):
        y = rng.standard_normal((n, 2)).astype(np.float32)
        got, table = check_against_model(pdt, 800 * H, y, 2, ppm=20000.0, residual=-123.456)
        assert len({fc.period(H, r, 20000.0) for r in range(-2, 3)}) == 5
    for k in range(4):
        y = np.zeros((40 * 4 + k, 2), np.float32)
        y[[17 + k, 22 + k, 90, 97, 133, 140], [1, 0, 1, 0, 1, 0]] = [1.0, 2.0, 0.5, 4.0, 1.0, 2.0]
        check_against_model(pdt, 3200, y, 2, ppm=20000.0)


def test_a_stream_longer_than_two_seconds_is_cut(pdt):
    rng = np.random.default_rng(3)
    y = rng.standard_normal((2 * 3200 + 500, 2)).astype(np.float32)
    a, b = pdt.host_ff_bits(3200, y, rate_steps=1, residual_hz=10.0), pdt.host_ff_bits(3200, y[: 2 * 3200], rate_steps=1, residual_hz=10.0)
    assert fc.same_bits(a, b) and 795 <= len(a.bits) <= 800
    assert a.index[-1] <= 2 * 3200


def test_mix(pdt):
    """the identity at residual 0; at +-496.5 Hz within 1e-6 |y| of a double rotation by the same step: the figure
    tests/test_channel_input.py holds the mixer's rotation of a unit impulse to"""
    rng = np.random.default_rng(9)
    fs, n = 32000, 70000
    y = rng.standard_normal((n, 2)).astype(np.float32)
    assert pdt.host_ff_mix(fs, 0.0, y).tobytes() == y.tobytes()
    z = y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)
    for f in (496.5, -496.5):
        step = round(f * 2 ** 32 / fs) % 2 ** 32
        p = (np.arange(n, dtype=np.uint64) * np.uint64(step)) % np.uint64(2 ** 32)
        want = z * np.exp(-2j * np.pi * p.astype(np.float64) / 2.0 ** 32)
        v = pdt.host_ff_mix(fs, f, y)
        err = np.abs((v[:, 0].astype(np.float64) + 1j * v[:, 1]) - want)
        print("mix at", f, "Hz: largest error / |y| =", (err / np.abs(z)).max())
        assert (err <= 1e-6 * np.abs(z)).all()


@pytest.mark.parametrize("mirrored", (False, True))
@pytest.mark.parametrize("R", (0, 20))
def test_the_real_recording_uncut(pdt, mirrored, R):
    """packet.wav whole: the chain never locks on it (real_captures.TABLE: lock -1) and its message is found only once the file is cut by
    hand.  Tone, feed-forward bits and either message rule give exactly one complete message, the recording's."""
    rate, _ = rc.capture("packet")
    assert all(rc.TABLE[k][0] == -1 for k in rc.TABLE if k[0] == "packet" and k[1] == rc.ARGOS)
    y = fc.real(mirrored)
    tone = pdt.host_tones(rate, 0.0, y, cap=1)
    assert len(tone) == 1 and tone[0]["valid"] and abs(abs(tone[0]["residual_hz"]) - 496.5) < 1.0
    assert (tone[0]["residual_hz"] > 0) == mirrored
    got = pdt.host_ff_bits(rate, y, rate_steps=R)
    assert got.sync["residual_hz"] == tone[0]["residual_hz"] and got.sync["tone_valid"] == 1
    assert fc.same_bits(got, pdt.host_ff_bits(rate, y, rate_steps=R, residual_hz=float(tone[0]["residual_hz"])))
    for rule in (0, 1):
        assert fc.decoded(pdt, got.bits, rule) == [fc.REAL_MESSAGE + (0 if mirrored else 1,)]
        m = pdt.host_argos_messages(got.bits.tobytes(), rule=rule)
        assert len(m) == 1 and m[0]["bit_index"] == 97


def test_bursts_at_a_wrong_bit_rate_need_the_grid(pdt):
    """eight blocks at 400 bit/s (1 + e): every e decodes at R = 20; e = +0.4 % does not at R = 0 (304 bits slip by more than one)"""
    fs = fc.BURST_FS
    for e in fc.RATE_ERRORS:
        y = fc.burst(e)
        got = pdt.host_ff_bits(fs, y)
        print("rate error", e, "-> r", int(got.sync["rate"]), "tau", int(got.sync["tau"]), "residual", float(got.sync["residual_hz"]))
        assert got.sync["tone_valid"] == 1 and abs(got.sync["residual_hz"] - 37.3) < 1.0
        assert fc.burst_decodes(pdt, got.bits), e
        assert abs(int(got.sync["rate"]) * 625e-6 + e) < 2 * 625e-6, e                  # a longer period for a slower burst
    assert fc.burst_decodes(pdt, pdt.host_ff_bits(fs, fc.burst(0.0), rate_steps=0).bits)
    assert not fc.burst_decodes(pdt, pdt.host_ff_bits(fs, fc.burst(0.004), rate_steps=0).bits)


@pytest.fixture(scope="module")
def pair(pdt):
    return bc.kind2_pair(pdt, (202, 206), 6.0)


def test_host_window_pipeline_loses_none(pdt, pair):
    """seeds (202, 206), 6 s -- the capture with the window at frame 4 620 288 that the chain loses under either rule:
    host_bursts -> burst_windows -> host_ddc -> host_ff_bits -> host_argos_messages gives 8 of 8 windows right under rule 0, none wrong"""
    x, params = pair
    _, _, _, found = pdt.host_bursts(bc.IN_RATE, bc.ARGOS_RANGE, bc.FS, x, rows=False)
    win = pdt.burst_windows(found, bc.IN_RATE, len(x))
    assert len(win) == 8 and 4620288 in [w.first_frame for w in win]
    msgs = []
    for w in win:
        y = pdt.host_ddc(bc.IN_RATE, bc.D, w.offset_hz, x[w.first_frame: w.first_frame + w.nframes])
        got = pdt.host_ff_bits(bc.FS, y)
        assert got.sync["tone_valid"] == 1
        msgs.append(pdt.host_argos_messages(got.bits.tobytes()))
    right, wrong, lost = bc.tally(pdt, params, win, msgs)
    print("windows right:", right, "of", len(win), "wrong:", wrong)
    assert (right, wrong, lost) == (8, 0, [])


def test_arguments(pdt):
    L = pdt.lib()
    y = np.zeros((100, 2), np.float32)
    sync, count = np.zeros(1, pdt.FF_SYNC_DTYPE), C.c_uint64(0)

    def host(rate, cfg, iq=y, n=100, s=sync, c=count):
        return L.pdt_host_ff_bits(rate, iq.ctypes.data if iq is not None else None, n, C.byref(cfg) if cfg is not None else None,
                                  s.ctypes.data if s is not None else None, None, None, None, 0, C.byref(c) if c is not None else None)

    assert host(3200, None) == 0 and count.value == 12
    for rate in (0, 800, 2400, 3201, 3200 - 800, 800 * 129, 44100):
        assert host(rate, None) == -1, rate
    assert host(800 * 128, None) == 0 and host(3200, pdt.FfCfg(rate_steps=32)) == 0
    for bad in (pdt.FfCfg(rate_steps=-1), pdt.FfCfg(rate_steps=33), pdt.FfCfg(rate_step_ppm=-1.0), pdt.FfCfg(rate_step_ppm=float("nan")),
                pdt.FfCfg(rate_step_ppm=float("inf")), pdt.FfCfg(rate_steps=20, rate_step_ppm=5001.0), pdt.FfCfg(flags=2),
                pdt.FfCfg(flags=1, residual_hz=float("nan")), pdt.FfCfg(flags=1, residual_hz=1600.0), pdt.FfCfg(flags=1, residual_hz=-1600.0)):
        assert host(3200, bad) == -1
    assert host(3200, pdt.FfCfg(flags=0, residual_hz=float("nan"))) == 0            # not given: not looked at
    assert host(3200, pdt.FfCfg(rate_steps=20, rate_step_ppm=4999.0)) == 0
    assert host(3200, None, iq=None) == -1 and host(3200, None, iq=None, n=0) == 0 and count.value == 0
    assert host(3200, None, s=None) == -1 and host(3200, None, c=None) == -1
    # rate_steps 0 means the default unless its flag bit is set
    z = np.random.default_rng(1).standard_normal((400, 2)).astype(np.float32)
    assert fc.same_bits(pdt.host_ff_bits(3200, z, residual_hz=0.0), pdt.host_ff_bits(3200, z, rate_steps=20, rate_step_ppm=625.0, residual_hz=0.0))
    cfg = pdt.FfCfg(rate_steps=0, flags=1)
    assert host(3200, cfg, iq=z, n=400) == 0
    assert sync[0].tobytes() == pdt.host_ff_bits(3200, z, rate_steps=20, residual_hz=0.0).sync.tobytes()
    # a stream shorter than the tone's segment, and a rate without an allowed segment: residual 0, not valid
    for fs, n in ((32000, 4000), (3200, 4000)):
        got = pdt.host_ff_bits(fs, np.ones((n, 2), np.float32), rate_steps=0)
        assert (got.sync["residual_hz"], got.sync["tone_valid"], got.sync["step"]) == (0.0, 0, 0)
    # the mixer's own arguments
    out = np.zeros((100, 2), np.float32)
    assert L.pdt_host_ff_mix(3200, 0.0, y.ctypes.data, 100, out.ctypes.data) == 0
    assert L.pdt_host_ff_mix(0, 0.0, y.ctypes.data, 100, out.ctypes.data) == -1
    assert L.pdt_host_ff_mix(3200, 1600.0, y.ctypes.data, 100, out.ctypes.data) == -1
    assert L.pdt_host_ff_mix(3200, float("nan"), y.ctypes.data, 100, out.ctypes.data) == -1
    assert L.pdt_host_ff_mix(3200, 0.0, None, 100, out.ctypes.data) == -1 and L.pdt_host_ff_mix(3200, 0.0, y.ctypes.data, 100, None) == -1
    assert L.pdt_host_ff_mix(3200, 0.0, None, 0, None) == 0
    assert C.sizeof(pdt.FfCfg) == 32 and C.sizeof(pdt.FfSync) == 48
