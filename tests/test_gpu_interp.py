"""The POES chain at the interpolation factors nothing else in the suite reaches: rint(150000 / rate) = 4 (37 500 Hz), 6 (25 000),
7 (22 050) and 9 (17 000), and the two half-way rates 60 000 (2.5 -> 2) and 20 000 (7.5 -> 8).  The factor picks the instantiation
of the register-tiled filter k_fir_interp_rt<float, I, 26> (I = 1 ... 8: separately unrolled code, its own LDS size and AGC tile
map), hands the filter to the generic k_fir_interp from 9 up -- although the plan had counted on the register-tiled form's AGC maps
--, and sets the grid of the stream segments.  Every comparison is byte for byte against the oracle; pdt_dev_fir_form
(Demodulator.fir_form) says which filter kernel ran and how many AGC maps it wrote.

    factor   rates in the suite (Hz)
    1        250 000, 200 000, 160 000, 150 000
    2        100 000, 96 000, 62 500, 60 000
    3        50 000, 48 000
    4        37 500
    5        32 000
    6        25 000
    7        22 050
    8        20 000, 18 750
    9        17 000
"""
import functools
import importlib
import os

import numpy as np
import pytest

from conftest import golden_text
from test_gpu_parity import assert_stage_equal, check_all_stages

pytestmark = pytest.mark.gpu

TILE = 64 * 26                    # inputs of one tile of the register-tiled filter
FIR_PLAIN, FIR_MIX, FIR_RT, FIR_GENERIC = 1, 2, 3, 4       # pdt_dev_fir_form (include/pdt_dev.h)
FACTOR = {60000: 2, 37500: 4, 25000: 6, 22050: 7, 20000: 8, 17000: 9, 50000: 3}


@functools.lru_cache(maxsize=None)
def capture(fs, secs=3.0, seed=1234):
    """A synthetic capture and its oracle, made once and shared (nobody writes to either)."""
    pdt = importlib.import_module("project-desert-tortoise_amd")
    from oracle import binding as orc
    iq = pdt.synth_capture(0, fs, secs, seed=seed)
    iq.setflags(write=False)
    return iq, orc.Oracle(orc.POES, fs, iq)


def with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def tiles_of(n):
    return (n + TILE - 1) // TILE


@pytest.mark.parametrize("fs", [37500, 25000, 22050, 17000, 60000, 20000])
def test_every_stage_at_every_new_rate(pdt, orc, fs):
    """The golden capture (3 s, seed 1234) at each new rate: every stage and the reference's text, and the filter kernel the factor
    is meant to take -- the register-tiled form with its AGC maps for 2 ... 8; at 9 the plan counts on those maps (the rotated taps
    exist and ntaps = 26 interp), the dispatch falls through to the generic kernel and the AGC makes its own."""
    iq, o = capture(fs)
    interp = FACTOR[fs]
    assert o.interp == interp == round(150000 / fs)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        assert d.fir_form() == (0, 0)
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        assert d.text() == golden_text(f"poes_{fs}.txt")
        s = d.stats()
        assert s.interp == interp and s.ntaps == 26 * interp
        form, tiles = d.fir_form()
        if interp <= 8:
            assert form == FIR_RT and tiles > 0, (form, tiles)
        else:
            assert (form, tiles) == (FIR_GENERIC, 0)


# (the stage entry puts the 26 inputs of the carried ring in front of the new ones: 1 637 ... 1 639 new inputs end around the first
# tile's edge as the kernel counts them, 1 663 ... 1 665 as the caller does)
@pytest.mark.parametrize("fs", [37500, 25000, 22050, 17000])
def test_filter_alone_at_the_edges_of_its_tile(pdt, orc, fs):
    """pdt_stage_fir on the oracle's PLL output: single calls on a fresh state whose lengths end just in front of, on and behind the
    first taps, the first tile (1 664 inputs) and a fourth one, then the whole stream with the ring carried from call to call in
    pieces of 1 (the first 2 000 inputs), 777, 1 664 and 10 000."""
    iq, o = capture(fs)
    interp = FACTOR[fs]
    x = o.stage(orc.ST_PLL)
    want = o.stage(orc.ST_FIR)
    assert len(want) == len(x) * interp
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        for n in (0, 1, 25, 26, 27, 1637, 1638, 1639, 1663, 1664, 1665, 3 * TILE + 7):
            assert_stage_equal(f"fir, one call of {n}", d.stage_fir(x[:n]), want[:n * interp])
        for piece in (1, 777, TILE, 10000):
            total = 2000 if piece == 1 else len(x)
            st = pdt.FirState()
            got = np.concatenate([d.stage_fir(x[a:a + piece], st) for a in range(0, total, piece)])
            assert_stage_equal(f"fir, pieces of {piece}", got, want[:total * interp])
            assert st.count == total


@pytest.mark.parametrize("n", [0, 1, 5, 77, 1663, 1664, 1665, 9999, 10000, 10001])
def test_short_captures_at_factor_7(pdt, orc, n):
    """22 050 Hz, the head of the golden capture: partial tiles, the zero padding of the tile's inputs in LDS, a fused AGC map over
    fewer outputs than a tile has, chunk lengths around the default chunk."""
    fs = 22050
    iq = capture(fs)[0][:n]
    o = orc.Oracle(orc.POES, fs, iq)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        assert d.fir_form() == ((FIR_RT, tiles_of(n)) if n else (0, 0))


def test_a_workgroups_second_tile(pdt, orc):
    """22 050 Hz with one filter workgroup per CU (PDT_FIR_WG_PER_CU=1: a grid of 256): 300 whole tiles and one of 221 inputs, so
    that 45 workgroups go round a second time and one of them ends on the partial tile."""
    fs, n = 22050, TILE * 300 + 221
    iq = pdt.synth_capture(0, fs, 23.0, seed=77)[:n]
    assert len(iq) == n
    o = orc.Oracle(orc.POES, fs, iq)

    def run():
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            assert d.fir_form() == (FIR_RT, 301)
    with_env({"PDT_FIR_WG_PER_CU": "1"}, run)


@pytest.mark.parametrize("fs", [22050, 25000])
@pytest.mark.parametrize("switch", ["PDT_FIR_GENERIC", "PDT_AGC_UNFUSED", "PDT_AGC_LANES"])
def test_alternative_kernels_at_a_new_factor(pdt, orc, fs, switch):
    """The generic filter, the AGC's own maps behind the register-tiled filter, and the per-lane AGC walkers on the filter's maps."""
    iq, o = capture(fs)

    def run():
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            return d.fir_form()
    form, tiles = with_env({switch: "1"}, run)
    if switch == "PDT_FIR_GENERIC":
        assert (form, tiles) == (FIR_GENERIC, 0)
    elif switch == "PDT_AGC_UNFUSED":
        assert (form, tiles) == (FIR_RT, 0)
    else:
        assert (form, tiles) == (FIR_RT, tiles_of(len(iq)))


@pytest.mark.parametrize("fs", [22050, 17000])
@pytest.mark.parametrize("blocks", [[2400], [1, 77, 9999, 30011], [12345, 3]])
def test_streams_at_factors_7_and_9(pdt, orc, fs, blocks):
    """The golden capture pushed in cycled block patterns: frames, text, totals, lock and norm factor equal the oracle's."""
    iq, o = capture(fs)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.stream_begin()
        i = k = 0
        got = []
        while i < len(iq):
            b = blocks[k % len(blocks)]
            got.append(d.stream_push(iq[i:i + b]))
            i += b
            k += 1
        got.append(d.stream_end())
        fr = np.concatenate(got)
        assert pdt.format_frames(fr) == o.text() == d.text()
        s = d.stats()
        ns, nsym, nbits, nfr = o.totals()
        assert (s.samples, s.symbols, s.bits, s.frames) == (ns, nsym, nbits, nfr)
        assert s.lock_sample == o.lock_sample and f"{s.lock_freq_hz:0.2f}" == f"{o.lock_freq_hz:0.2f}"
        assert np.float32(s.norm_factor) == np.float32(o.norm_factor)
        assert d.fir_form()[0] == (FIR_GENERIC if fs == 17000 else FIR_RT)


@pytest.mark.parametrize("chunk", [1664, 1000])
def test_aligned_segments_at_factor_4(pdt, orc, chunk):
    """37 500 Hz in pushes of 208 000 samples = 125 filter tiles, 3 pushes and 12 345 samples.  A segment may take the whole-capture
    kernels when its first new output lies on a run of 208 outputs and a 128-byte line, and the filter writes the AGC's tile maps in
    it when that output is also the first of a tile of 64 * 26 * 4 -- both counted from the WINDOW's origin, not the stream's.  The
    window slides to the last multiple of lcm(chunk, 26) that leaves the history (0.63 s + 8 192 = 31 817 samples) in front of the
    next new sample, and segments end on whole chunks.  With chunk = 1 000 a later segment therefore begins at a local sample h, a
    multiple of 1 000 with 31 817 <= h < 44 817, which is never a multiple of 1 664 (lcm(1 000, 1 664) = 208 000), whatever the size
    of the pushes: here h = 39 000, on the run and line grid (156 000 outputs = 750 runs) but inside a tile, so only the stream's
    first segment gets the filter's maps.  The smallest chunk that keeps every segment on the tile grid is 1 664 (lcm(1 664, 26) =
    1 664: origin and segment ends are whole tiles, h = 33 280 = 20 tiles); it is run with the same pushes, and the chunk of 1 000
    beside it.  After every push the window's newest filter and AGC outputs are the oracle's, bit for bit; PDT_SEG_PLAIN keeps the
    stream path's kernels and gives the same text."""
    fs, block, interp = 37500, 208000, 4
    n = 3 * block + 12345
    iq = pdt.synth_capture(0, fs, 17.0, seed=91)[:n]
    assert len(iq) == n
    o = orc.Oracle(orc.POES, fs, iq, chunk=chunk)
    ofir, oagc = o.stage(orc.ST_FIR), o.stage(orc.ST_AGC)

    def run(check_stages):
        forms = []
        with pdt.Demodulator(pdt.MODE_POES, fs, chunk=chunk) as d:
            d.stream_begin()
            got, done = [], 0
            for i in range(0, n, block):
                got.append(d.stream_push(iq[i:i + block]))
                forms.append(d.fir_form())
                prev, done = done, min(i + block, n) // chunk * chunk          # whole reference chunks so far
                # (the window has already slid when the push returns: the AGC's tail was copied down over the window's older part,
                # at least 169 000 samples = 676 000 outputs from its end after a full push, the new chunks' worth after the last one)
                new = min((done - prev) * interp, 600000)
                if check_stages:
                    for st, want in ((pdt.ST_FIR, ofir), (pdt.ST_AGC, oagc)):
                        a = d.stage(st)
                        assert new > 0 and len(a) >= new
                        assert_stage_equal(f"stage {st} after the push at {i}", a[len(a) - new:], want[done * interp - new:done * interp])
            got.append(d.stream_end())
            assert pdt.format_frames(np.concatenate(got)) == o.text() == d.text()
            assert d.stats().frames == len(o.frames()) >= 150
        return forms

    forms = run(True)
    assert len(forms) == 4 and all(f[0] == FIR_RT for f in forms), forms
    assert forms[0][1] == 125
    if chunk == 1664:
        assert forms[2][1] > 0 and all(f[1] > 0 for f in forms), forms          # the last full push, and every other one
    else:
        assert [f[1] for f in forms[1:]] == [0, 0, 0], forms
    plain = with_env({"PDT_SEG_PLAIN": "1"}, lambda: run(False))
    assert all(f == (FIR_RT, 0) for f in plain), plain


def test_one_batch_of_five_rates(pdt, orc):
    """pdt_demod_batch_device takes contexts of different rates (captures whose plans differ in shape do not share launches, they
    run one group after the other): factors 4, 6, 7, 9 and 3 in one call, every stage of each against its oracle."""
    import torch
    cases = [(37500, 3.0, 61), (25000, 4.0, 62), (22050, 3.0, 63), (17000, 5.0, 64), (50000, 3.0, 65)]
    caps = [capture(fs, secs, seed) for fs, secs, seed in cases]
    dev = [torch.from_numpy(iq.reshape(-1).copy()).to("cuda:0") for iq, _ in caps]
    torch.cuda.synchronize()
    ds = [pdt.Demodulator(pdt.MODE_POES, fs) for fs, _, _ in cases]
    try:
        pdt.demod_batch(ds, [t.data_ptr() for t in dev], [len(iq) for iq, _ in caps])
        for d, (iq, o), (fs, _, _) in zip(ds, caps, cases):
            check_all_stages(pdt, orc, d, o)
            assert d.stats().interp == FACTOR[fs]
            assert d.fir_form() == ((FIR_GENERIC, 0) if fs == 17000 else (FIR_RT, tiles_of(len(iq))))
    finally:
        for d in ds:
            d.close()
