"""The chain on silence, full scale, NaN and infinity: the captures of tests/degenerate_cases.py through every entry of
the C ABI -- whole captures at every geometry, the alternative kernels, streams, the bounded window, the stage entries, a batch --
against the oracle, which tests/test_degenerate.py pins on the reference's own objects for the same captures.  The rule is
degenerate_cases': every NaN one value, everything else byte for byte, every element of every stream.

Why the loops these inputs reach end when a sample or a state is a NaN or an infinity (read before the first run):
  * k_pll_fix: every round with an open seam commits at least one re-run and moves `from` behind it; the cascade's r only grows; both
    stop at r_hi.  Seams are compared with bits_equal throughout (pll_rewalk's checkpoints too), so a NaN state equals itself, and a
    re-run records the very bits it started from: the seam it leaves is closed whatever the value.  pll_core's two wrap loops
    (`while phase > 2 pi`) would spin on an infinite phase, and cannot get one: theta = arctan2_ref is a NaN or within +-pi (its
    quotient is a NaN or within [-1, 1]), the frequency is clamped (a NaN passes both compares), the error is theta - phase wrapped
    once, so the phase is a NaN -- both loop tests false -- or bounded.
  * k_pll_tail: one for loop over the blocks from the stretch's start, r++ in every path, to nb.
  * k_agc_fix: r = rb + 1 behind every repair and r += 64 where 64 seams are closed, to nb; bits_equal on the gains.  agc_step's
    clamps let a NaN gain through, as the reference's do; agc_calm takes a NaN sample for calm and both steps give a NaN gain.
  * k_gardner_ring's walker on a staged chunk with s_bad set: the plain loop, whose checked step tests rint(ns) < n -- false for a
    NaN -- and whose check-free batch is counted (K from a finite ns, at most OUT - nout); an index converted from a NaN is 0.  The
    stagers wait for s_done, which the walker sets after every walked chunk whatever it held.  A chunk without a walk: ns ==
    memo_in and gs == rint(gs) are false for a NaN, the plain loop's test is false at once.  k_calm_emit: the same test.
  * the table, span and four-per-wavefront emission kernels clip with v_med3_f32, which gives a bound for a NaN error, and take
    their indices from the bits of the sampling instant (rint_index, lds_rel_at: NOT 0 for a NaN), so they must never hold a NaN
    instant, and do not: they start from candidates (finite by construction) or from recorded states of such walks; a window
    that held a NaN or an infinity (k_gardner_table_merge) or an unclipped error that is one (k_gardner_span_walk) is marked beside
    the states (a flag bit, bit 31 of the record's symbol count, a missing tail), never in them; k_gardner_emit_first zeroes an
    entry state that is not finite before it walks, for the sub-groups that only shadow a group too, and leaves such a group,
    and every group whose key has no tail, to the checked walker.  Finite instants advance by at least step - lim a symbol, so every walk
    leaves its window.  A state the chain cannot key (gardner_encode_exit: mf == (float)m is false for a NaN) is
    PDT_GTAB_MISS; the key searches are binary searches over unsigned keys (lo < hi shrinks whatever the key); a miss is walked
    by k_gardner_chain, whose c grows in every path.
  * gardner_walk_chunk: the checked step's test is false for a NaN; room > 0 is false for a NaN, so K = 0; the window moves only
    while the chunk is not done.
  * k_mm: rint(next) < n is false for a NaN; a NaN step passes both clamps and makes next a NaN; an infinite sample gives an
    infinite or NaN error, the step is clamped into [step_min, step_max] or a NaN: next advances by at least step_min or ends.
  * k_chunk_need: one strided for loop over two chunks; it compares bit patterns, so a NaN or -0.0 needs a walk.

What the first run found (no loop failed to end; two results were wrong, both fixed with this file):
  * that median is also why the table sampler was wrong: its walks went on over a NaN where the reference's instant becomes a NaN
    and the capture's symbols end -- 29 627 symbols for the reference's 1 on p50-zero-chunk0, 29 809 for 16 642 on
    p50-nan-after-lock, 9 298 for 5 992 on p250-nan, 48 806 for 24 268 on live-nan.  Windows that hold a NaN or an infinity, and
    walks that meet an error that is one, are flagged; flagged chunks are left untabulated and walked with the checked step alone
    (DESIGN 4.1).
  * k_static_gain's bracketing chains forgot a NaN in front of the chunk's last 192 samples: p50-nan-before-lock had a finite norm
    factor and 300 finite AGC samples where the reference has NaN.  The NaN is now kept as the chunk's maximum.
"""
import os

import numpy as np
import pytest

import degenerate_cases as dc

pytestmark = pytest.mark.gpu

NAN_CASE, INF_CASE, GAP_CASE = "p50-nan-after-lock", "p50-zero-chunk0", "p50-mid-silence"
SMALL_BLOCKS = dict(pll_block=256, pll_warm=256, agc_block=64, agc_warm=64)        # every seam a repaired seam


def with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def run_case(pdt, orc, name, pll_kept=True, **kw):
    _, mode, fs, chunk, chain, a, _ = dc.case(name)
    o = dc.oracle(name)                                   # (asserts the case's own property first)
    with pdt.Demodulator(mode, fs, chunk=chunk, chain=chain, **kw) as d:
        if not pll_kept:
            d.keep_pll(False)
        if mode == pdt.MODE_ARGOS:
            d.keep_presquelch()
        d.demod_raw(a) if a.dtype.kind == "f" else d.demod(a)
        dc.check_all_stages(pdt, orc, d, o, pll_kept)
        if mode == pdt.MODE_ARGOS:
            dc.assert_stream_equal("agc before squelch", d.stage(pdt.ST_AGC_RAW), o.stage(orc.ST_AGC_RAW))
        return d.stats()


# ---------------------------------------------------------------- 1, 2: whole captures, every stage
@pytest.mark.parametrize("name", [c[0] for c in dc.cases()])
def test_whole_capture_every_stage(pdt, orc, name):
    """POES 50 ksps at the default chunk and at 3 333, 250 ksps (k_mix_fir), the live chain, ARGOS; the pair 9 999 / 10 000 zeros and
    the single LSB at the edge of k_static_gain's underflow are among them"""
    st = run_case(pdt, orc, name)
    if name.startswith("p250"):
        assert st.interp == 1


@pytest.mark.parametrize("name", [c[0] for c in dc.cases() if c[0].startswith("p250")])
def test_250ksps_without_the_pll_stream(pdt, orc, name):
    """INTERP 1 in the lean mode: the PLL stream never goes through HBM, what remains is compared"""
    run_case(pdt, orc, name, pll_kept=False)


# ---------------------------------------------------------------- 3: alternative kernels
@pytest.mark.parametrize("name", [NAN_CASE, INF_CASE, GAP_CASE])
@pytest.mark.parametrize("switch", ["PDT_FIR_GENERIC", "PDT_AGC_UNFUSED", "PDT_AGC_LANES", "PDT_GARDNER_SEQUENTIAL", "PDT_PLL_NOCKPT",
                                    "PDT_PLL_NOTAIL"])
def test_alternative_kernels(pdt, orc, switch, name):
    with_env({switch: "1"}, lambda: run_case(pdt, orc, name))


@pytest.mark.parametrize("name", ["p50-nan-after-lock-c3333", "p50-zero-3333-c3333", "p250-nan", "p250-zero-chunk0"])
@pytest.mark.parametrize("env", [{"PDT_GSPAN": "3", "PDT_GSPAN_REKEY": "0"}, {"PDT_GSPAN": "4", "PDT_GSPAN_REKEY": "1"},
                                 {"PDT_GSPAN": "3", "PDT_GEMIT_GROUPS": "1"}])
def test_table_rows_of_several_chunks(pdt, orc, env, name):
    """rows of three and four chunks (k_gardner_span_walk in one stage and with the re-key point behind a row's second chunk,
    k_gardner_emit_first / _rest, and the wavefront-per-group emission): at chunks of 3 333 the stream's first NaN is the 15th sample
    of chunk 15 -- the last chunk of the row 12 .. 15, behind its re-key point, or the first of the row 15 .. 17; at 250 ksps it is the first sample of chunk 9, the
    first chunk of a row of three; the all-NaN streams have it in front of everything"""
    st = with_env(env, lambda: run_case(pdt, orc, name))
    assert st.gardner_parallel == 1


@pytest.mark.parametrize("name", ["argos-zero-chunk0", "argos-mid-silence"])
def test_argos_without_the_stride(pdt, orc, name):
    with_env({"PDT_GARDNER_NOSTRIDE": "1"}, lambda: run_case(pdt, orc, name))


@pytest.mark.parametrize("name", [NAN_CASE, INF_CASE, GAP_CASE])
def test_small_blocks_every_seam_repaired(pdt, orc, name):
    st = run_case(pdt, orc, name, **SMALL_BLOCKS)
    assert st.agc_seam_fixes > 0


# ---------------------------------------------------------------- 4: streams
@pytest.mark.parametrize("name", [NAN_CASE, INF_CASE, GAP_CASE])
@pytest.mark.parametrize("blocks", [[2400], [1, 77, 9999, 30011], [12345, 3]])
def test_streams_carry_the_state(pdt, orc, blocks, name):
    """a NaN or infinite state is carried from segment to segment: text, totals, lock and norm factor are the oracle's"""
    _, mode, fs, chunk, chain, a, _ = dc.case(name)
    o = dc.oracle(name)
    with pdt.Demodulator(mode, fs, chunk=chunk, chain=chain) as d:
        d.stream_begin()
        i = k = 0
        got = []
        while i < len(a):
            b = blocks[k % len(blocks)]
            got.append(d.stream_push(a[i:i + b]))        # (pdt_stream_push_f32 for a float32 array)
            i += b
            k += 1
        got.append(d.stream_end())
        assert pdt.format_frames(np.concatenate(got)) == o.text()
        dc.check_results(pdt, d, o)


# ---------------------------------------------------------------- 5: the bounded window
@pytest.mark.parametrize("name", [GAP_CASE, NAN_CASE])
def test_bounded_window(pdt, orc, name):
    """chunks of 2 000 and pieces of 32 000 samples (a piece is at least 16 chunks): four pieces"""
    _, mode, fs, _, chain, a, expect = dc.case(name)
    o = orc.Oracle(mode, fs, a, chunk=2000)
    dc.check_expectations(orc, o, expect)

    def run():
        with pdt.Demodulator(mode, fs, chunk=2000) as d:
            d.demod_raw(a) if a.dtype.kind == "f" else d.demod(a)
            st = d.stats()
            assert st.windowed == 1 and st.segments >= 3, (st.windowed, st.segments)
            dc.check_results(pdt, d, o)
    with_env({"PDT_WINDOW_PIECE": "32000"}, run)


# ---------------------------------------------------------------- 6: stage entries
def chunks_of(n, chunk):
    return [(a, min(a + chunk, n)) for a in range(0, n, chunk)]


def same_fields(a, b, fields):
    for f in fields:
        assert dc.same_number(float(getattr(a, f)), float(getattr(b, f))), (f, getattr(a, f), getattr(b, f))


def test_stage_pll_on_samples_with_a_nan(pdt, orc):
    from test_gpu_stages import pll_replay
    _, mode, fs, _, _, x, _ = dc.case(NAN_CASE)
    o = dc.oracle(NAN_CASE)
    with pdt.Demodulator(mode, fs) as d:
        out, lock, rets, st = pll_replay(pdt, d, x, 10000)
        dc.assert_stream_equal("pll", out, o.stage(orc.ST_PLL))
        dc.assert_stream_equal("avg", rets.astype("<f4"), o.stage(orc.ST_AVG)[:len(rets)])
        assert st.started == 1 and st.locked == 1 and st.lock_index == o.lock_sample % 10000
        assert np.isnan(st.phase) and np.isnan(out[-1])
        out2, lock2, _, st2 = pll_replay(pdt, d, x, 33333)             # another cut: the same streams, the same record
        dc.assert_stream_equal("pll, other cut", out2, out)
        dc.assert_stream_equal("lock, other cut", lock2, lock)
        same_fields(st, st2, ("started", "locked", "lock_freq_hz", "phase", "freq", "avg_phase", "locksig", "sweep"))


def test_stage_fir_on_nan_and_on_both_infinities(pdt, orc):
    o = dc.oracle(NAN_CASE)
    x, want = o.stage(orc.ST_PLL), o.stage(orc.ST_FIR)
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        st = pdt.FirState()
        got = np.concatenate([d.stage_fir(x[a:b], st) for a, b in chunks_of(len(x), 10000)])
        dc.assert_stream_equal("fir", got, want)
        assert st.count == len(x) and np.isnan(np.array(st.history[:26])).all()
        # +inf and -inf nine samples apart, both under the 26 input taps at once; then each alone
        y = x[:1500].copy()
        y[700], y[709], y[1100], y[1300] = np.inf, -np.inf, np.inf, -np.inf
        model = dc.fir_interp_model(y, o.stage(orc.ST_TAPS), o.interp)
        assert dc.nan_count(model) > 0 and np.isposinf(model).any() and np.isneginf(model).any()
        for cut in (1500, 705, 64):
            st = pdt.FirState()
            got = np.concatenate([d.stage_fir(y[a:b], st) for a, b in chunks_of(len(y), cut)])
            dc.assert_stream_equal(f"fir on infinities, pieces of {cut}", got, model)


def test_stage_agc_from_an_infinite_gain_and_over_a_nan(pdt, orc):
    for name, kw in ((INF_CASE, {}), (NAN_CASE, {}), (INF_CASE, dict(agc_block=64, agc_warm=64)), (NAN_CASE, dict(agc_block=64, agc_warm=64))):
        o = dc.oracle(name)
        x, want = o.stage(orc.ST_FIR), o.stage(orc.ST_AGC)
        with pdt.Demodulator(pdt.MODE_POES, 50000, **kw) as d:
            st = pdt.AgcState()
            got = np.concatenate([d.stage_agc(x[a:b], o.norm_factor, st) for a, b in chunks_of(len(x), 30000)])
            dc.assert_stream_equal(f"agc {name}", got, want)
            whole = pdt.AgcState()
            dc.assert_stream_equal(f"agc {name}, one call", d.stage_agc(x, o.norm_factor, whole), want)
            assert st.started == 1 and np.isnan(st.gain)
            same_fields(st, whole, ("started", "gain"))
    # the first NaN ends a calm stretch: the 64 samples in front of it are within +-1 and the gain there within [2.5, 4000]
    o = dc.oracle(NAN_CASE)
    x, y = o.stage(orc.ST_FIR), o.stage(orc.ST_AGC)
    first = int(np.flatnonzero(np.isnan(x))[0])
    assert np.abs(x[first - 64:first]).max() <= 1.0 and 2.5 <= abs(y[first - 1] / x[first - 1]) <= 4000.0


def test_stage_squelch_and_static_gain(pdt, orc):
    _, mode, fs, _, _, a, _ = dc.case("argos-zero-chunk0")
    o = dc.oracle("argos-zero-chunk0")
    raw, lock, want = o.stage(orc.ST_AGC_RAW), o.stage(orc.ST_LOCK), o.stage(orc.ST_AGC)
    assert dc.nan_count(raw) > dc.nan_count(want) > 0                 # the squelch zeroes some of the NaN, not all
    with pdt.Demodulator(mode, fs) as d:
        sq = np.concatenate([d.stage_squelch(raw[i:j], lock[i:j], 0.15) for i, j in chunks_of(len(raw), 2400)])
        dc.assert_stream_equal("squelch", sq, want)
        assert d.stage_static_gain(a[:2400]) == o.norm_factor == np.inf
    zeros = np.zeros((10000, 2), dtype="<i2")
    lsb = zeros.copy()
    lsb[5000] = (1, 0)
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        assert d.stage_static_gain(zeros) == np.inf and d.stage_static_gain(lsb) == np.inf
        assert d.stage_static_gain(dc.as_float(zeros)) == np.inf
        iq = dc.case("p50-zero-9999")[5]
        assert np.float32(d.stage_static_gain(iq[:10000])) == np.float32(dc.oracle("p50-zero-9999").norm_factor)
        nanf = dc.case("p50-nan-before-lock")[5]
        assert np.isnan(d.stage_static_gain(nanf[:10000])) and np.isnan(dc.oracle("p50-nan-before-lock").norm_factor)


@pytest.mark.parametrize("name", [INF_CASE, "p50-nan-after-lock-c3333", NAN_CASE, "argos-zero-chunk0"])
def test_stage_gardner_on_nan_streams(pdt, orc, name):
    """an AGC stream that is NaN throughout, one that becomes NaN in the middle of a chunk (chunks of 3 333: sample 150 000 is the
    15th of its chunk) and at a chunk's first sample, and the ARGOS form with the lock array behind the buffer"""
    from test_gpu_stages import gardner_replay
    _, mode, fs, chunk, _, _, _ = dc.case(name)
    o = dc.oracle(name)
    x = o.stage(orc.ST_AGC)
    C = (chunk or (2400 if mode == pdt.MODE_ARGOS else 10000)) * o.interp
    with pdt.Demodulator(mode, fs, chunk=chunk) as d:
        sym, pick, st = gardner_replay(pdt, d, x, C, lock=o.stage(orc.ST_LOCK) if mode == pdt.MODE_ARGOS else None)
        dc.assert_stream_equal("sym", sym, o.stage(orc.ST_SYM))
        dc.assert_stream_equal("symidx", pick, o.stage(orc.ST_SYMIDX))
        assert dc.same_number(st.prev_bit, float(sym[-1]))
        assert np.isnan(st.next_sample) == bool(dc.nan_count(x))
        # the carried record, field by field: in front of the first NaN's chunk against the oracle's picks (nextSample = the next
        # pick's instant rolled over, so its rint is that pick's index), at the end against a second replay
        first_bad = int(np.flatnonzero(np.isnan(x))[0]) // C
        if first_bad > 0:
            st1 = pdt.GardnerState()
            buf = np.zeros(C, dtype=x.dtype)
            lock = o.stage(orc.ST_LOCK) if mode == pdt.MODE_ARGOS else None
            nbuf = np.zeros(C, dtype=x.dtype) if lock is not None else None
            for i in range(first_bad):
                buf[:] = x[i * C:(i + 1) * C]
                if nbuf is not None:
                    nbuf[:] = lock[i * C:(i + 1) * C]
                d.stage_gardner(buf, C, st1, nbuf)
            want_idx = o.stage(orc.ST_SYMIDX)
            nxt = want_idx[want_idx >= first_bad * C]
            assert np.isfinite([st1.next_sample, st1.prev_bit, st1.half_sample]).all()
            if len(nxt):
                assert int(np.rint(st1.next_sample)) == int(nxt[0]) - first_bad * C
            before = o.stage(orc.ST_SYM)[want_idx < first_bad * C]
            assert st1.prev_bit == float(before[-1])
        _, _, st2 = gardner_replay(pdt, d, x, C, lock=o.stage(orc.ST_LOCK) if mode == pdt.MODE_ARGOS else None)
        same_fields(st, st2, ("next_sample", "prev_bit", "half_sample"))


@pytest.mark.parametrize("name", [INF_CASE, "p50-nan-after-lock-c3333", "argos-zero-chunk0"])
def test_stage_mm_on_nan_streams(pdt, orc, name):
    _, mode, fs, chunk, _, a, _ = dc.case(name)
    o = orc.Oracle(mode, fs, a, chunk=chunk, sampler=1)
    x = o.stage(orc.ST_AGC)
    dc.assert_stream_equal("the sampler's input", x, dc.oracle(name).stage(orc.ST_AGC))
    step = (chunk or (2400 if mode == pdt.MODE_ARGOS else 10000)) * o.interp
    with pdt.Demodulator(mode, fs, chunk=chunk, sampler=1) as d:
        st = pdt.MmState()
        syms, picks = [], []
        for i, j in chunks_of(len(x), step):
            s, p = d.stage_mm(x[i:j], st)
            syms.append(s)
            picks.append(p.astype(np.int64) + i)
        syms = np.concatenate(syms)
        dc.assert_stream_equal("sym", syms, o.stage(orc.ST_SYM))
        dc.assert_stream_equal("symidx", np.concatenate(picks), o.stage(orc.ST_SYMIDX))
        assert st.started == 1 and dc.same_number(st.sample_last, float(syms[-1]))
        st2 = pdt.MmState()                                  # a second replay: the same record, field by field
        for i, j in chunks_of(len(x), step):
            d.stage_mm(x[i:j], st2)
        same_fields(st, st2, ("started", "next_sample", "step_size", "sample_last"))
        # ... and the whole capture with that sampler
        d.demod_raw(a) if a.dtype.kind == "f" else d.demod(a)
        dc.check_all_stages(pdt, orc, d, o)


def test_stage_manchester_on_symbols_with_a_nan(pdt, orc):
    from test_gpu_stages import manchester_replay
    o = dc.oracle(NAN_CASE)
    sym, symidx = o.stage(orc.ST_SYM), o.stage(orc.ST_SYMIDX)
    assert dc.nan_count(sym) == 1
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        bits, bsym, st = manchester_replay(pdt, d, sym, symidx, 10000 * o.interp, 1.0)
        assert bits.tobytes() == o.stage(orc.ST_BITS).tobytes()
        dc.assert_stream_equal("bit times", o.stage(orc.ST_SYMT)[bsym], o.stage(orc.ST_BITT))
        assert st.even_odd == len(sym) % 256 and dc.same_number(st.current, float(sym[-1])) and dc.same_number(st.previous, float(sym[-2]))
        b1, k1 = d.stage_manchester(sym, 1.0)
        assert b1.tobytes() == bits.tobytes() and np.array_equal(k1.astype(np.int64), bsym)


# ---------------------------------------------------------------- 7: a batch
def test_batch_degenerate_slots_beside_healthy_ones(pdt, orc):
    """a healthy capture, the one with an infinite norm factor (its AGC stream is NaN throughout), the mid-silence one, the all-zero
    one and another healthy one share every launch; each slot equals its own oracle at every stage.  pdt_demod_batch_device takes
    int16 captures, which cannot hold a NaN sample: the mid-silence capture stands where the float capture with a NaN would"""
    import torch
    names = ["p50-clean", INF_CASE, GAP_CASE, "p50-all-zero", "p50-full-scale-runs"]
    caps = [dc.case(n)[5] for n in names]
    dev = [torch.from_numpy(a.reshape(-1).copy()).to("cuda:0") for a in caps]
    torch.cuda.synchronize()
    ds = [pdt.Demodulator(pdt.MODE_POES, 50000) for _ in caps]
    try:
        pdt.demod_batch(ds, [t.data_ptr() for t in dev], [len(a) for a in caps])
        for n, d in zip(names, ds):
            dc.check_all_stages(pdt, orc, d, dc.oracle(n))
    finally:
        for d in ds:
            d.close()
