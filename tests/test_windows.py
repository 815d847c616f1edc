"""Every burst of a wideband capture in a window of its own, without a GPU: pdt_burst_windows against its formulas,
and the whole route on the host -- burst search, windows, the down-converter's restatement on each slice, the oracle's ARGOS chain
-- on the two-platform capture of tests/test_gpu_bursts.py: every payload sent is decoded, the first burst of each platform included,
and nothing else.  That pins the inputs on which the GPU test's figure (tests/test_gpu_windows.py) is safe."""
import ctypes as C
import math

import numpy as np
import pytest

IN_RATE, D = 1024000, 32
FS = IN_RATE // D
ARGOS_RANGE = 550.0
OFFSETS = (250000.0, -333300.0)
SEEDS = (8, 9)
RESIDUAL = 120.0
PERIOD_S = 1.5                                                             # the synthetic platforms send every 1.5 s


def llround(v: float) -> int:
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def platforms(pdt, in_rate: int, secs: float, offsets, seeds, residual: float):
    """Transmissions summed into one int16 capture, each at half amplitude, carrier i at offsets[i] + residual (the capture of
    tests/test_gpu_channel_input.py's carriers())."""
    n = int(round(secs * in_rate))
    total = np.zeros((n, 2), dtype=np.int32)
    params = []
    for off, seed in zip(offsets, seeds):
        p = pdt.synth_params(1, in_rate, off + residual, seed)
        p.amplitude //= 2
        p.noise_gain //= 2
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
        total += iq
        params.append(p)
    return np.clip(total, -32768, 32767).astype(np.int16), params


def to_cu8(x16: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(x16 / 256.0) + 128, 0, 255).astype(np.uint8)


def expected_payload(pdt, params, offsets, residual, w, in_rate) -> bytes:
    """The payload of the burst a window was cut for: the platform nearest its offset, the burst nearest its start."""
    near = int(np.argmin([abs(w.offset_hz - (off + residual)) for off in offsets]))
    return bytes(pdt.synth_argos_payload(params[near], int(round(w.first_frame / in_rate / PERIOD_S))))


def some_bursts(pdt):
    B = pdt.Burst
    return [B(0, 12, 0.0, 0.384, 250120.0, 30.0, 1.0), B(47, 13, 1.504, 0.416, -333180.0, 28.0, 1.0), B(450, 11, 14.4, 0.352, 1234.5, 20.0, 1.0),
            B(460, 12, 14.72, 0.384, -5.0, 20.0, 1.0)]


def test_burst_windows_defaults(pdt):
    bursts = some_bursts(pdt)
    cap = int(15.0 * IN_RATE)
    win = pdt.burst_windows(bursts, IN_RATE, cap)
    assert len(win) == len(bursts)
    for b, w in zip(bursts, win):
        first = llround((b.start_s + b.duration_s / b.rows) * IN_RATE)
        end = min(cap, llround((b.start_s + b.duration_s + 0.1) * IN_RATE))
        assert (w.first_frame, w.nframes, w.offset_hz) == (first, end - first, b.offset_hz)
    assert win[0].first_frame == 32768 and win[3].first_frame + win[3].nframes == cap      # one row of 8 x 4096; cut at the capture's end


def test_burst_windows_explicit_skip_and_tail(pdt):
    bursts = some_bursts(pdt)
    cap = int(15.0 * IN_RATE)
    for skip, tail in ((0.0, 0.0), (0.05, 0.25), (0.0123, 1.0), (-1.0, 0.0), (0.0, -1.0)):
        win = pdt.burst_windows(bursts, IN_RATE, cap, skip, tail)
        for b, w in zip(bursts, win):
            s = b.duration_s / b.rows if skip < 0 else skip
            t = 0.1 if tail < 0 else tail
            first = llround((b.start_s + s) * IN_RATE)
            end = min(cap, llround((b.start_s + b.duration_s + t) * IN_RATE))
            assert (w.first_frame, w.nframes, w.offset_hz) == (first, max(end - first, 0), b.offset_hz)


def test_burst_windows_that_are_empty(pdt):
    b = some_bursts(pdt)[1]
    cap = int(15.0 * IN_RATE)
    assert pdt.burst_windows([b], IN_RATE, cap, b.duration_s, 0.0)[0].nframes == 0          # skip = duration: start reaches end
    assert pdt.burst_windows([b], IN_RATE, cap, 2.0, 0.0)[0].nframes == 0                   # ... and beyond it
    assert pdt.burst_windows([b], IN_RATE, int(1.0 * IN_RATE))[0].nframes == 0              # a capture that ends before the burst
    assert pdt.burst_windows([], IN_RATE, cap) == []


def test_burst_windows_arguments(pdt):
    L = pdt.lib()
    rec = (pdt.BurstRec * 1)(pdt.BurstRec(*some_bursts(pdt)[0]))
    out = (pdt.WindowRec * 1)()
    assert L.pdt_burst_windows(rec, 1, IN_RATE, 1000000, -1.0, -1.0, out) == 0
    assert L.pdt_burst_windows(None, 1, IN_RATE, 1000000, -1.0, -1.0, out) == -1
    assert L.pdt_burst_windows(rec, 1, IN_RATE, 1000000, -1.0, -1.0, None) == -1
    assert L.pdt_burst_windows(None, 0, IN_RATE, 1000000, -1.0, -1.0, None) == 0
    assert L.pdt_burst_windows(rec, -1, IN_RATE, 1000000, -1.0, -1.0, out) == -1
    assert L.pdt_burst_windows(rec, 1, 0, 1000000, -1.0, -1.0, out) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.pdt_burst_windows(rec, 1, IN_RATE, 1000000, bad, -1.0, out) == -1
        assert L.pdt_burst_windows(rec, 1, IN_RATE, 1000000, -1.0, bad, out) == -1
        for field in ("start_s", "duration_s", "offset_hz"):
            r = (pdt.BurstRec * 1)(pdt.BurstRec(*some_bursts(pdt)[0]))
            setattr(r[0], field, bad)
            assert L.pdt_burst_windows(r, 1, IN_RATE, 1000000, -1.0, -1.0, out) == -1


def test_window_record_layout(pdt):
    assert C.sizeof(pdt.WindowRec) == 24


@pytest.fixture(scope="module")
def argos_pair(pdt):
    return platforms(pdt, IN_RATE, 15.0, OFFSETS, SEEDS, RESIDUAL)


@pytest.mark.parametrize("rendering", ("int16", "cu8"))
def test_host_pipeline_decodes_every_burst(pdt, orc, argos_pair, rendering):
    """host_bursts -> burst_windows -> host_ddc of each slice, rendered as int16 -> the oracle's ARGOS chain: the 20 payloads sent,
    each in the window cut for its burst, and nothing that was not sent."""
    x16, params = argos_pair
    x = x16 if rendering == "int16" else to_cu8(x16)
    _, _, _, found = pdt.host_bursts(IN_RATE, ARGOS_RANGE, FS, x, rows=False)
    nb = int(len(x) / IN_RATE / PERIOD_S)
    sent = {bytes(pdt.synth_argos_payload(p, b)) for p in params for b in range(nb)}
    assert len(found) == 2 * nb == 20
    win = pdt.burst_windows(found, IN_RATE, len(x))
    hit, extra = 0, 0
    for w in win:
        y = pdt.host_ddc(IN_RATE, D, w.offset_hz, x[w.first_frame: w.first_frame + w.nframes])
        y16 = np.clip(np.round(y.reshape(-1, 2) * 32768.0), -32768, 32767).astype(np.int16)
        o = orc.Oracle(orc.ARGOS, FS, y16)
        got = [bytes(f.bytes[:7]) for f in o.frames() if f.complete]
        hit += expected_payload(pdt, params, OFFSETS, RESIDUAL, w, IN_RATE) in got
        extra += sum(g not in sent for g in got)
    print(rendering, "windows with their payload:", hit, "of", len(win), "payloads not sent:", extra)
    assert hit == 20 and extra == 0
