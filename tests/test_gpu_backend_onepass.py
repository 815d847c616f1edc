"""The symbol back end in its chip-wide form: the one-pass Manchester decision (k_manch_onepass, decoupled look-back over
4096-symbol tiles) and the frame filter over batches of sync hits (k_sync_dense / k_sync_links / k_sync_mark).  Both are
checked against the oracle and against the kernels they replace, which stay behind the developer switches
PDT_MANCH_3PASS (tile summaries, one-workgroup scan, emission) and PDT_SYNC_SERIAL (one-workgroup filter)."""
import os

import numpy as np
import pytest

from test_gpu_bytesync import SYNC_POES, check, inv

pytestmark = pytest.mark.gpu

SWITCHES = [None, "PDT_MANCH_3PASS", "PDT_SYNC_SERIAL"]


def fast_bits(rng, n):
    return (rng.integers(0, 2, size=n, dtype=np.uint8) + ord("0")).tobytes().decode()


def run(pdt, mode, rate, iq, switch):
    if switch:
        os.environ[switch] = "1"
    try:
        with pdt.Demodulator(mode, rate) as d:
            d.demod(iq)
            s = d.stats()
            return (d.text(), d.frames_array(), d.stage(pdt.ST_BITS), d.stage(pdt.ST_BITSYM),
                    (s.symbols, s.bits, s.frames, s.sync_overflow))
    finally:
        if switch:
            del os.environ[switch]


@pytest.mark.parametrize("mode", ["poes", "argos"])
def test_switches_give_the_same_outputs(pdt, orc, mode):
    """A capture of a few hundred Manchester tiles (several look-back windows of 64), decided by the one-pass kernel, by
    the three passes, and framed by the serial filter: the same bits, bit time stamps, frames and counts, equal to the
    oracle's."""
    if mode == "poes":
        rate, iq = 50000, pdt.synth_capture(0, 50000, 40.0, seed=907)
        o = orc.Oracle(orc.POES, rate, iq, keep_stages=False)
        m = pdt.MODE_POES
    else:
        rate, iq = 32000, pdt.synth_capture(1, 32000, 30.0, f0_hz=120.0, seed=908)
        o = orc.Oracle(orc.ARGOS, rate, iq, keep_stages=False, math_mode=orc.MATH_LIBM)
        m = pdt.MODE_ARGOS
    ref = run(pdt, m, rate, iq, None)
    assert ref[0] == o.text()
    assert ref[4][2] == len(o.frames())
    assert ref[4][1] > 2 * 4096
    for sw in SWITCHES[1:]:
        got = run(pdt, m, rate, iq, sw)
        assert got[0] == ref[0], sw
        assert np.array_equal(got[1], ref[1]), sw
        assert np.array_equal(got[2], ref[2]), sw
        assert np.array_equal(got[3], ref[3]), sw
        assert got[4] == ref[4], sw


def test_quiet_stretches_carry_the_clock_across_tiles(pdt, orc, clip):
    """Stretches of zeros (no resynchronisation for many tiles: the tile maps pass the incoming clock through) between
    copies of the clip: the clockmod and the bit count must cross every tile boundary as the oracle's do."""
    rate, iq = clip
    gap = np.zeros((rate * 3, 2), dtype=iq.dtype)
    cap = np.ascontiguousarray(np.concatenate([iq, gap, iq[: rate * 2], gap, iq]))
    o = orc.Oracle(orc.POES, rate, cap)
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        d.demod(cap)
        assert np.array_equal(d.stage(pdt.ST_BITS), o.stage(orc.ST_BITS))
        assert d.text() == o.text()


def test_frame_filter_over_many_batches(pdt, orc):
    """About 30 000 frames: the dense hit list spans eight batches of 4096 (and four of the serial filter's LDS batches),
    with sync words inside open frames, inverse frames and gaps, so that batch entries fall on every kind of hit."""
    rng = np.random.default_rng(23)
    parts = [fast_bits(rng, 211)]
    for i in range(30000):
        body = fast_bits(rng, 813)
        if i % 89 == 0:
            body = body[:300] + SYNC_POES + body[319:]          # ignored: inside the frame
        if i % 37 == 0:
            parts.append(inv(SYNC_POES) + inv(body))
        else:
            parts.append(SYNC_POES + body)
        if i % 11 == 0:
            parts.append(fast_bits(rng, int(rng.integers(1, 60))))
    s = "".join(parts)
    ov, n = check(pdt, orc, pdt.MODE_POES, s)
    assert ov == 0 and n >= 30000
    os.environ["PDT_SYNC_SERIAL"] = "1"
    try:
        ov2, n2 = check(pdt, orc, pdt.MODE_POES, s)
    finally:
        del os.environ["PDT_SYNC_SERIAL"]
    assert (ov2, n2) == (ov, n)
