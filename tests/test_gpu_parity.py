"""Parity of the HIP path (through the C ABI) with the oracle -- the tests proper.

Bit-exact at every stage: PLL output, FIR output, AGC output (float32 bit patterns), Gardner
symbols and their sample indices, Manchester bits, frame bytes, and the output-file text
including the %.5f time stamps.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import bits_equal

from conftest import GOLDEN, ROOT, golden_text

pytestmark = pytest.mark.gpu


def assert_stage_equal(name, g, o):
    assert len(g) == len(o), f"{name}: length {len(g)} vs {len(o)}"
    if g.tobytes() != o.tobytes():
        gv = g.view(np.uint8).reshape(len(g), -1)
        ov = o.view(np.uint8).reshape(len(o), -1)
        first = int(np.flatnonzero((gv != ov).any(axis=1))[0])
        raise AssertionError(f"{name}: first difference at {first}: gpu {g[first:first+3]} oracle {o[first:first+3]}")


def check_all_stages(pdt, orc, d, o):
    assert_stage_equal("pll", d.stage(pdt.ST_PLL), o.stage(orc.ST_PLL))
    if d.mode == pdt.MODE_ARGOS:
        assert_stage_equal("lock", d.stage(pdt.ST_LOCK), o.stage(orc.ST_LOCK))
    assert_stage_equal("fir", d.stage(pdt.ST_FIR), o.stage(orc.ST_FIR))
    assert_stage_equal("agc", d.stage(pdt.ST_AGC), o.stage(orc.ST_AGC))
    assert_stage_equal("sym", d.stage(pdt.ST_SYM), o.stage(orc.ST_SYM))
    assert_stage_equal("symidx", d.stage(pdt.ST_SYMIDX), o.stage(orc.ST_SYMIDX))
    assert_stage_equal("bits", d.stage(pdt.ST_BITS), o.stage(orc.ST_BITS))
    assert d.text() == o.text()
    s = d.stats()
    ns, nsym, nbits, nfr = o.totals()
    assert (s.samples, s.symbols, s.bits, s.frames) == (ns, nsym, nbits, nfr)
    assert s.lock_sample == o.lock_sample
    if o.lock_sample >= 0:
        assert f"{s.lock_freq_hz:0.2f}" == f"{o.lock_freq_hz:0.2f}"
    if d.mode == pdt.MODE_ARGOS:
        assert s.norm_factor == o.norm_factor
    else:
        assert np.float32(s.norm_factor) == np.float32(o.norm_factor)


@pytest.mark.parametrize("chunk", [0, 1000, 3333, 260000])
def test_clip_all_stages(pdt, orc, clip, chunk):
    rate, iq = clip
    o = orc.Oracle(orc.POES, rate, iq, chunk=chunk)
    with pdt.Demodulator(pdt.MODE_POES, rate, chunk=chunk) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        if chunk in (0, 1000):
            assert d.text() == golden_text("clip.c10000.txt")
            assert hashlib.md5(d.text()).hexdigest() == "d3c496d003a29eeee061c01b00ce025c"      # SURVEY 8c golden
        if chunk == 260000:
            assert d.text() == golden_text("clip.c260000.txt")


def test_clip_norm_override(pdt, orc, clip):
    rate, iq = clip
    with pdt.Demodulator(pdt.MODE_POES, rate, norm_override=12.5) as d:
        d.demod(iq)
        assert d.text() == golden_text("clip.n12.txt")


@pytest.mark.parametrize("fs", [17000, 18750, 20000, 22050, 25000, 32000, 37500, 50000, 60000, 100000, 250000])
def test_synthetic_rates_golden(pdt, orc, golden, fs):
    p = golden["params"]
    iq = pdt.synth_capture(0, fs, p["poes_seconds"], seed=p["poes_seed"])
    assert hashlib.sha256(iq.tobytes()).hexdigest() == golden["synth"][f"poes_{fs}"]
    o = orc.Oracle(orc.POES, fs, iq)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        assert d.text() == golden_text(f"poes_{fs}.txt")


@pytest.mark.parametrize("kw", [
    dict(pll_block=4000, pll_warm=8000, agc_block=12000, agc_warm=90000),     # many seams
    dict(pll_block=64, pll_warm=64, agc_block=64, agc_warm=64),               # warm-up far too short: every seam repaired
    dict(pll_block=1 << 30, pll_warm=0, agc_block=1 << 30, agc_warm=0),       # one block: purely sequential
])
def test_block_geometry_never_changes_the_result(pdt, orc, clip, kw):
    rate, iq = clip
    iq = iq[:120000]
    o = orc.Oracle(orc.POES, rate, iq)
    with pdt.Demodulator(pdt.MODE_POES, rate, **kw) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        if kw["pll_block"] == 64:
            assert d.stats().pll_seam_fixes > 0 and d.stats().agc_seam_fixes > 0


@pytest.mark.parametrize("switch", ["", "PDT_PLL_NOSHORT", "PDT_PLL_NOCKPT", "PDT_PLL_NOCONSENSUS"])
def test_early_walkers_checkpoints_consensus_never_change_the_result(pdt, orc, switch):
    """Round 4's additions to the block-parallel PLL, each switched off in turn, on a geometry where all of them act: 97 blocks
    of 4 096 samples with a warm-up of five blocks and 512 samples -- the early walkers get their own workgroup (their first
    tracking segment is 2 846 samples, everybody else's 512), the warm-up is short enough for open seams (re-runs that stop at
    a checkpoint), and the noise (x4) loses a walker now and then (consensus)."""
    import ctypes as C
    fs = 50000
    p = pdt.synth_params(0, fs, 1000.0, 4242)
    p.noise_gain = int(p.noise_gain * 4)
    n = 97 * 4096 + 1234
    iq = np.zeros((n, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
    o = orc.Oracle(orc.POES, fs, iq)
    if switch:
        os.environ[switch] = "1"
    try:
        with pdt.Demodulator(pdt.MODE_POES, fs, pll_block=4096, pll_warm=5 * 4096 + 512) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
    finally:
        os.environ.pop(switch, None)


@pytest.mark.parametrize("n", [0, 1, 5, 77, 9999, 10000, 10001, 20000, 25000])
def test_short_and_ragged_captures(pdt, orc, clip, n):
    """empty input, less than one chunk, exact multiples of the chunk (Q7), ragged tail"""
    rate, iq = clip
    part = iq[30000:30000 + n]
    o = orc.Oracle(orc.POES, rate, part)
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        d.demod(part)
        check_all_stages(pdt, orc, d, o)


def test_noise_only_never_locks(pdt, orc):
    rng = np.random.default_rng(5)
    iq = rng.integers(-400, 400, size=(150000, 2)).astype(np.int16)
    o = orc.Oracle(orc.POES, 50000, iq)
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)


def test_negative_and_large_carrier_offsets(pdt, orc):
    for f0, seed in ((-3100.0, 21), (4200.0, 22), (12.0, 23)):
        iq = pdt.synth_capture(0, 50000, 4.0, f0_hz=f0, seed=seed)
        o = orc.Oracle(orc.POES, 50000, iq)
        with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)


def test_inverted_frames(pdt, orc):
    """I/Q swapped -> the PLL locks on the mirrored spectrum and frames arrive through the inverse sync word."""
    iq = pdt.synth_capture(0, 50000, 5.0, seed=31)[:, ::-1].copy()
    o = orc.Oracle(orc.POES, 50000, iq)
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)


@pytest.mark.parametrize("seed,f0,secs,chunk", [(99, 120.0, 13.0, 0), (12, -90.0, 20.0, 1000), (13, 60.0, 24.0, 2401),
                                                (14, 199.0, 16.0, 4800), (15, 140.0, 9.0, 20000)])
def test_argos_all_stages(pdt, orc, golden, seed, f0, secs, chunk):
    """ARGOS chain (double): bit-exact against the oracle in its portable-math mode (the mode that
    tests/test_oracle_ref.py ties to the reference's packet output), incl. the lock-signal stream,
    Squelch, the heap-adjacency reads of the Gardner seam (Q16) and odd/even/huge chunk sizes."""
    iq = pdt.synth_capture(1, 32000, secs, f0_hz=f0, seed=seed)
    o = orc.Oracle(orc.ARGOS, 32000, iq, chunk=chunk, math_mode=orc.MATH_LIBM)
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000, chunk=chunk) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        assert d.stats().frames >= 5
        if seed == 99:
            assert d.text() == golden_text("argos_32000.txt")           # the reference's own output
            par = pdt.synth_params(1, 32000, f0, seed)
            fr = d.frames_array()
            sent = [bytes(pdt.synth_argos_payload(par, b)) for b in range(9)]
            assert [bytes(f["bytes"][:7]) for f in fr] == sent          # round trip: all 9 bursts, payload exact


@pytest.mark.parametrize("fs,chunk", [(32000, 2400), (32000, 2401), (32000, 1999), (44100, 2400), (32001, 2400), (48000, 777), (50000, 2500)])
def test_argos_squelched_chunks_in_one_stride(pdt, orc, fs, chunk):
    """Chunks whose samples are all +0.0 behind Squelch need no walk: the sampler only adds its step (k_chunk_need).  Round 5:
    where the sampling instant and the step are multiples of 2^(E - 53) below 2^E -- step 40.0 at 32 ksps, 55.125 at 44.1 ksps,
    62.5 at 50 ksps; after every roll-over of a chunk of 2 048 samples or more -- those additions are exact and the chunk is taken
    in one stride (k_gardner_ring); 32 001 sps has a step that is no such multiple and keeps the additions one by one, a chunk of
    1 999 or 777 samples rolls over below the top binade and strides only once the instant has been rounded there, an odd chunk
    length has its last pick on a tie.  Same symbols, pick indices and packets as the oracle either way, and with the stride
    switched off."""
    import os
    iq = pdt.synth_capture(1, fs, 24.0, f0_hz=130.0, seed=41)
    o = orc.Oracle(orc.ARGOS, fs, iq, chunk=chunk, math_mode=orc.MATH_LIBM)
    for env in ({}, {"PDT_GARDNER_NOSTRIDE": "1"}):
        os.environ.update(env)
        try:
            with pdt.Demodulator(pdt.MODE_ARGOS, fs, chunk=chunk) as d:
                d.demod(iq)
                check_all_stages(pdt, orc, d, o)
                assert d.stats().symbols > 0
        finally:
            for k in env:
                os.environ.pop(k, None)


def test_argos_block_geometry_and_short_inputs(pdt, orc):
    iq = pdt.synth_capture(1, 32000, 8.0, f0_hz=120.0, seed=5)
    o = orc.Oracle(orc.ARGOS, 32000, iq, math_mode=orc.MATH_LIBM)
    for kw in (dict(pll_block=8000, pll_warm=16000, agc_block=8000, agc_warm=16000),
               dict(pll_block=256, pll_warm=256, agc_block=256, agc_warm=256)):
        with pdt.Demodulator(pdt.MODE_ARGOS, 32000, **kw) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
    for n in (0, 3, 2399, 2400, 2401, 4800):
        part = iq[:n]
        o2 = orc.Oracle(orc.ARGOS, 32000, part, math_mode=orc.MATH_LIBM)
        with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as d:
            d.demod(part)
            check_all_stages(pdt, orc, d, o2)


def test_cli_demodargos(pdt, tmp_path, golden):
    p = golden["params"]
    iq = pdt.synth_capture(1, 32000, p["argos_seconds"], seed=p["argos_seed"])
    wav = tmp_path / "argos.wav"
    pdt.write_wav(str(wav), 32000, iq)
    out = tmp_path / "packets.txt"
    r = subprocess.run([os.path.join(ROOT, "bin", "demodARGOS"), "-o", str(out), str(wav)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == golden_text("argos_32000.txt")
    assert golden_text("argos_32000.txt").decode() in r.stdout          # packets are mirrored to stdout (ARGOSdemod/ByteSync.c)


@pytest.mark.parametrize("chunk,kw", [(0, {}), (1000, {}), (0, dict(agc_block=256, agc_warm=256))])
def test_argos_presquelch_stream_and_cli_raw_dump(pdt, orc, tmp_path, chunk, kw):
    """ARGOSdemod -r (main.c:171-180,273-274): output.raw receives the AGC output BEFORE Squelch, chunk after chunk.
    The stream is kept on request (pdt_keep_presquelch, stage ST_AGC_RAW) and must equal the oracle's, which
    tests/test_oracle_ref.py compares with the reference's own objects; the host program writes it with -r."""
    iq = pdt.synth_capture(1, 32000, 10.0, f0_hz=150.0, seed=77)
    o = orc.Oracle(orc.ARGOS, 32000, iq, chunk=chunk, math_mode=orc.MATH_LIBM)
    want = o.stage(orc.ST_AGC_RAW)
    assert len(want) == len(iq) and (want != o.stage(orc.ST_AGC)).any()          # the squelch does act on this capture
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000, chunk=chunk, **kw) as d:
        d.demod(iq)
        assert d.stage(pdt.ST_AGC_RAW).size == 0                                  # not kept unless asked for
        d.keep_presquelch().demod(iq)
        assert d.stage(pdt.ST_AGC_RAW).tobytes() == want.tobytes()
        check_all_stages(pdt, orc, d, o)
    if chunk == 0 and not kw:
        wav = tmp_path / "a.wav"
        pdt.write_wav(str(wav), 32000, iq)
        r = subprocess.run([os.path.join(ROOT, "bin", "demodARGOS"), "-r", "-o", str(tmp_path / "p.txt"), str(wav)], capture_output=True,
                           text=True, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        assert (tmp_path / "output.raw").read_bytes() == want.tobytes()
        assert (tmp_path / "p.txt").read_bytes() == o.text()


@pytest.mark.parametrize("scale", [1.0, 37.5, 0.004])
def test_raw_float32_input(pdt, orc, tmp_path, scale):
    """RAW float32 captures (pdt_demod_f32): bit-exact vs the oracle's RAW path, through the CLI too."""
    iq = pdt.synth_capture(0, 50000, 4.0, seed=5)
    raw = (iq.astype(np.float32) / np.float32(32768.0)) * np.float32(scale)
    o = orc.Oracle(orc.POES, 50000, raw)
    with pdt.Demodulator(pdt.MODE_POES, 50000) as d:
        d.demod_raw(raw)
        check_all_stages(pdt, orc, d, o)
        assert d.stats().frames >= 38
    path = tmp_path / "cap.raw"
    raw.tofile(path)
    out = tmp_path / "mf.txt"
    r = subprocess.run([os.path.join(ROOT, "bin", "demodPOES"), "-s", "50", "-o", str(out), str(path)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == o.text()
    r = subprocess.run([os.path.join(ROOT, "bin", "demodPOES"), "-o", str(out), str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "Sample Rate (in Khz) must be specified" in r.stdout
    with pytest.raises(pdt.PdtError):
        pdt.Demodulator(pdt.MODE_ARGOS, 32000).demod_raw(raw)        # the ARGOS program refuses RAW files


def test_context_reuse_and_device_input(pdt, orc, clip):
    import torch
    rate, iq = clip
    o_full = orc.Oracle(orc.POES, rate, iq, keep_stages=False)
    o_half = orc.Oracle(orc.POES, rate, iq[:100000], keep_stages=False)
    t = torch.from_numpy(iq.copy()).cuda()
    with pdt.Demodulator(pdt.MODE_POES, rate) as d:
        d.demod(iq)
        assert d.text() == o_full.text()
        d.demod(iq[:100000])                      # smaller capture on the same context
        assert d.text() == o_half.text()
        d.set_stream(torch.cuda.current_stream().cuda_stream)
        d.demod_device(t.data_ptr(), len(iq))     # input already resident in HBM
        assert d.text() == o_full.text()


def test_round_trip_two_minutes(pdt):
    """Size-independent property at a larger size: every complete decoded frame is one of the
    transmitted frames, consecutive, and nearly all of them arrive."""
    fs, secs, seed = 50000, 120.0, 4242
    iq = pdt.synth_capture(0, fs, secs, seed=seed)
    par = pdt.synth_params(0, fs, 1000.0, seed)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.demod(iq)
        fr = d.frames_array()
        st = d.stats()
    complete = fr[fr["complete"] == 1]
    assert len(complete) >= 1190
    sent = {bytes(pdt.synth_poes_frame(par, k)): k for k in range(0, 1210)}
    idx = [sent.get(bytes(f["bytes"])) for f in complete]
    assert all(i is not None for i in idx)
    assert idx == list(range(idx[0], idx[0] + len(idx)))
    # the warm-ups re-converge at (nearly) every seam; the rare miss is repaired, never wrong
    assert st.pll_seam_fixes <= st.pll_blocks // 50 and st.agc_seam_fixes <= st.agc_blocks // 50
    # time stamps: monotone apart from the documented zeros (Q2/Q4), 0.1 s frame period
    t = fr["time"][fr["time"] > 0]
    assert np.all(np.diff(t) > 0.09)


def test_ten_minute_capture_matches_oracle(pdt, orc):
    """BASELINE configs[1] at full size: 30 000 000 samples, bit-exact output file vs the CPU oracle."""
    fs = 50000
    iq = pdt.synth_capture(0, fs, 600.0, seed=1234)
    o = orc.Oracle(orc.POES, fs, iq, keep_stages=False)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.demod(iq)
        assert d.text() == o.text()
        assert d.stats().frames == len(o.frames()) >= 5990


@pytest.mark.parametrize("switch", ["PDT_FIR_GENERIC", "PDT_AGC_UNFUSED", "PDT_GARDNER_ONEBUF", "PDT_GARDNER_NORING", "PDT_EMA_NOGUESS",
                                    "PDT_GARDNER_SEQUENTIAL", "PDT_AGC_LANES"])
def test_alternative_kernels_agree(pdt, orc, clip, switch):
    """The generic kernel variants behind developer switches (tools/README.md) -- the fallbacks other geometries take by
    themselves -- give the same bits as the default path."""
    rate, iq = clip
    o = orc.Oracle(orc.POES, rate, iq)
    a = pdt.synth_capture(1, 32000, 8.0, f0_hz=150.0, seed=31)
    oa = orc.Oracle(orc.ARGOS, 32000, a, math_mode=orc.MATH_LIBM)
    os.environ[switch] = "1"
    try:
        with pdt.Demodulator(pdt.MODE_POES, rate) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
        with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as d:
            d.demod(a)
            check_all_stages(pdt, orc, d, oa)
    finally:
        del os.environ[switch]


@pytest.mark.parametrize("chunk", [601, 2399, 2400, 1200])
def test_ring_sampler_chunk_shapes(pdt, orc, chunk):
    """The ring sampler (k_gardner_ring: staged chunks several ahead of the walker, squelched chunks never read): odd chunk
    sizes (no 16-byte staging), a capture of zeros only (no chunk is walked), a capture whose squelch never closes for long,
    and the float build on a POES capture (PDT_GARDNER_SEQUENTIAL keeps it off the boundary-state tables)."""
    a = pdt.synth_capture(1, 32000, 21.0, f0_hz=-140.0, seed=77)
    for iq in (a, np.zeros_like(a[: 32000 * 4]), np.ascontiguousarray(np.tile(a[int(2.0 * 32000):int(2.9 * 32000)], (12, 1)))):
        o = orc.Oracle(orc.ARGOS, 32000, iq, chunk=chunk, math_mode=orc.MATH_LIBM)
        with pdt.Demodulator(pdt.MODE_ARGOS, 32000, chunk=chunk) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
    p = pdt.synth_capture(0, 50000, 3.0, seed=78)
    o = orc.Oracle(orc.POES, 50000, p, chunk=chunk)
    os.environ["PDT_GARDNER_SEQUENTIAL"] = "1"
    try:
        with pdt.Demodulator(pdt.MODE_POES, 50000, chunk=chunk) as d:
            d.demod(p)
            check_all_stages(pdt, orc, d, o)
            assert d.stats().frames > 20
    finally:
        del os.environ["PDT_GARDNER_SEQUENTIAL"]


@pytest.mark.parametrize("mult", [5, 10])
def test_weak_signal_repair_cascades(pdt, orc, mult):
    """Noise scaled up 5x / 10x (6 dB / 0 dB SNR): the tracking loop stops being contracting, many seams fail their
    bitwise check and are re-run in cascades -- every stage must still equal the oracle."""
    import ctypes as C
    fs, secs = 50000, 20.0
    p = pdt.synth_params(0, fs, 1000.0, 77)
    p.noise_gain = int(p.noise_gain * mult)
    n = int(round(secs * fs))
    iq = np.zeros((n, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
    o = orc.Oracle(orc.POES, fs, iq)
    # without the walkers' consensus (round 4: outliers behind the wide-band stage take their wavefront's median frequency) the
    # lost walkers are all there: the repair path, cascades and checkpoint exits included, really runs
    os.environ["PDT_PLL_NOCONSENSUS"] = "1"
    try:
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            lone = d.stats().pll_seam_fixes
            assert lone >= 5
    finally:
        del os.environ["PDT_PLL_NOCONSENSUS"]
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        assert d.stats().pll_seam_fixes <= lone       # (x5: 9 -> 2 on the round's build; the result is the same either way)


def test_250ksps_capture_matches_oracle(pdt, orc):
    """BASELINE configs[2]/[4] geometry (250 ksps, interp 1, 26 taps) on a 160-second, 40 000 000-sample capture -- past
    the point (128 s) where the reference's float32 running-sum time axis stalls at this rate, so the stalled
    time stamps are compared too: bit-exact output file vs the CPU oracle, every transmitted frame in order.
    (tests/test_gpu_long.py runs the full 60-minute / 900 M-sample capture against the reference's own objects.)"""
    fs, secs, seed = 250000, 160.0, 31
    iq = pdt.synth_capture(0, fs, secs, seed=seed)
    o = orc.Oracle(orc.POES, fs, iq, keep_stages=False)
    par = pdt.synth_params(0, fs, 1000.0, seed)
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:
        d.demod(iq)
        assert d.text() == o.text()
        fr = d.frames_array()
        st = d.stats()
    assert st.interp == 1 and st.ntaps == 26 and st.gardner_parallel == 1
    complete = fr[fr["complete"] == 1]
    assert len(complete) >= 1590
    assert sum(1 for f in complete if f"{f['time']:.5f}" == "128.00000") >= 300          # the stall (Q1)
    sent = {bytes(pdt.synth_poes_frame(par, k)): k for k in range(0, 1610)}
    idx = [sent.get(bytes(f["bytes"])) for f in complete]
    assert all(i is not None for i in idx) and idx == list(range(idx[0], idx[0] + len(idx)))


def test_spans_over_noise_and_overflowing_key_lists(pdt, orc):
    """Rows whose scouts do not settle (noise in front of the signal: the whole boundary-state domain is listed, thousands of
    distinct exits per row) go through the same three span kernels; with a key list too small for them (PDT_GSPAN_CAP) such rows
    are left untabulated, the chain walks them and the wavefront-per-group kernel emits them; PDT_GEMIT_GROUPS: that kernel for
    every group."""
    fs = 250000
    rng = np.random.default_rng(15)
    noise = np.clip(np.rint(rng.normal(0, 900, (int(1.0 * fs), 2))), -32768, 32767).astype("<i2")
    iq = np.ascontiguousarray(np.concatenate([noise, pdt.synth_capture(0, fs, 5.0, seed=48)]))
    o = orc.Oracle(orc.POES, fs, iq)
    for env in ({"PDT_GSPAN": "8"}, {"PDT_GSPAN": "8", "PDT_GSPAN_CAP": "2000"}, {"PDT_GSPAN": "3"},
                {"PDT_GSPAN": "4", "PDT_GEMIT_GROUPS": "1"}):
        os.environ.update(env)
        try:
            with pdt.Demodulator(pdt.MODE_POES, fs) as d:
                d.demod(iq)
                check_all_stages(pdt, orc, d, o)
                st = d.stats()
                assert st.gardner_parallel == 1 and st.gardner_full_domain > 0
                if "PDT_GSPAN_CAP" in env:
                    assert st.gardner_walked > 0
        finally:
            for k in env:
                del os.environ[k]


def test_chain_walks_into_a_row_and_takes_the_recorded_tail(pdt, orc):
    """A row whose entry state lies outside the scouts' band (a very narrow band on a weak capture): the chain walks the row's
    first chunk and, finding its exit among the distinct exits the span kernels walked on from, takes the rest of the row from
    there -- same symbols as ever."""
    import ctypes as C
    fs, secs = 250000, 24.0
    p = pdt.synth_params(0, fs, 1000.0, 91)
    p.noise_gain = int(p.noise_gain * 4)
    n = int(round(secs * fs))
    iq = np.zeros((n, 2), dtype="<i2")
    pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
    o = orc.Oracle(orc.POES, fs, iq)
    os.environ.update({"PDT_GSPAN": "4", "PDT_BAND_PAD": "0.002"})
    try:
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            assert d.stats().gardner_walked > 0, "no row entered outside its band on this capture: the path was not exercised"
    finally:
        del os.environ["PDT_GSPAN"], os.environ["PDT_BAND_PAD"]


@pytest.mark.parametrize("fs,secs,chunk,span", [(250000, 12.0, 0, 4), (250000, 12.0, 0, 16), (250000, 9.0, 2500, 7),
                                                (50000, 30.0, 1000, 16), (250000, 12.02, 0, 3), (100000, 6.0, 3000, 2)])
def test_table_rows_spanning_several_chunks(pdt, orc, fs, secs, chunk, span):
    """Boundary states tabulated in front of every span-th chunk only (k_gardner_span: what hour-long captures run by default,
    forced here through PDT_GSPAN on short ones): every stage equals the oracle -- spans that do not divide the number of
    chunks, a last group of one short chunk, small chunks."""
    iq = pdt.synth_capture(0, fs, secs, seed=300 + span)
    o = orc.Oracle(orc.POES, fs, iq, chunk=chunk)
    os.environ["PDT_GSPAN"] = str(span)
    try:
        with pdt.Demodulator(pdt.MODE_POES, fs, chunk=chunk) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            st = d.stats()
            assert st.gardner_parallel == 1 and st.frames > 20
            n_chunks = -(-len(iq) // (chunk or 10000))
            if chunk == 0:       # rows, not chunks, were tabulated (the default chunk: the scouts settle, every row has a short list)
                assert st.gardner_candidates < 2100 * ((n_chunks - 1) // span + 1)
    finally:
        del os.environ["PDT_GSPAN"]


@pytest.mark.parametrize("fs,secs,seed,kw", [(250000, 9.0, 41, {}), (200000, 3.3, 42, {}), (160000, 2.0, 43, {"chunk": 3333}),
                                             (250000, 0.0301, 44, {}), (250000, 4.0, 45, {"pll_block": 1664}),
                                             (250000, 4.0, 46, {"pll_block": 832, "pll_warm": 30000})])
def test_mix_and_filter_in_one_kernel(pdt, orc, fs, secs, seed, kw):
    """INTERP 1 captures take k_mix_fir (mix + FIR fused, the PLL output only in LDS): every stage equals the oracle -- with
    the PLL stream kept (the default) and, in the lean mode the host programs use, without it; the unfused pair of kernels
    behind PDT_MIX_UNFUSED gives the same bits.  Cases: lengths that end inside a run / a block / a tile, a capture shorter
    than one block, the smallest legal block sizes (every run next to a block boundary, seams repaired)."""
    iq = pdt.synth_capture(0, fs, secs, seed=seed)
    chunk = kw.get("chunk", 0)
    dkw = {k: v for k, v in kw.items() if k != "chunk"}
    o = orc.Oracle(orc.POES, fs, iq, chunk=chunk)
    with pdt.Demodulator(pdt.MODE_POES, fs, chunk=chunk, profile=True, **dkw) as d:
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        assert d.stats().interp == 1
        assert "mix_fir" in d.kernel_times() and "pll_mix" not in d.kernel_times()
        fir_kept = d.stage(pdt.ST_FIR)
        d.keep_pll(False)
        d.demod(iq)
        assert d.text() == o.text()
        assert bits_equal(d.stage(pdt.ST_FIR), fir_kept) and bits_equal(d.stage(pdt.ST_AGC), o.stage(orc.ST_AGC))
        assert len(d.stage(pdt.ST_PLL)) == 0
    os.environ["PDT_MIX_UNFUSED"] = "1"
    try:
        with pdt.Demodulator(pdt.MODE_POES, fs, chunk=chunk, profile=True, **dkw) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            assert "pll_mix" in d.kernel_times() and "mix_fir" not in d.kernel_times()
    finally:
        del os.environ["PDT_MIX_UNFUSED"]


def test_mix_fir_noise_only_and_late_lock(pdt, orc):
    """k_mix_fir takes the samples up to the lock from the acquisition's output: a capture that never locks (the whole
    stream), and one whose signal rises after a second of noise (the lock far inside the capture)."""
    fs = 250000
    rng = np.random.default_rng(5)
    noise = np.clip(np.rint(rng.normal(0, 900, (int(1.2 * fs), 2))), -32768, 32767).astype("<i2")
    sig = pdt.synth_capture(0, fs, 3.0, seed=47)
    for iq in (noise, np.ascontiguousarray(np.concatenate([noise[: fs], sig]))):
        o = orc.Oracle(orc.POES, fs, iq)
        with pdt.Demodulator(pdt.MODE_POES, fs, profile=True) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            assert "mix_fir" in d.kernel_times()
    assert o.lock_sample > fs


@pytest.mark.parametrize("rg,kp", [(0.0, 0.0), (9.0, 0.05)])
def test_mm_clock_recovery_poes(pdt, orc, clip, rg, kp):
    """MMClockRecovery as the sampler (cfg.sampler = 1); every stage against the oracle, whose M&M
    restatement is checked against the reference's own object in tests/test_oracle_ref.py."""
    rate, iq = clip
    o = orc.Oracle(orc.POES, rate, iq, sampler=1, mm_range=rg or 3.0, mm_kp=kp or 0.15)
    with pdt.Demodulator(pdt.MODE_POES, rate, sampler=pdt.SAMPLER_MM, mm_step_range=rg, mm_kp=kp) as d:
        d.demod(iq)
        assert d.stats().gardner_parallel == 0
        check_all_stages(pdt, orc, d, o)
    iq2 = pdt.synth_capture(0, 50000, 12.0, seed=8)
    o2 = orc.Oracle(orc.POES, 50000, iq2, chunk=3333, sampler=1, mm_range=rg or 3.0, mm_kp=kp or 0.15)
    with pdt.Demodulator(pdt.MODE_POES, 50000, chunk=3333, sampler=pdt.SAMPLER_MM, mm_step_range=rg, mm_kp=kp) as d:
        d.demod(iq2)
        check_all_stages(pdt, orc, d, o2)


def test_mm_clock_recovery_argos(pdt, orc):
    iq = pdt.synth_capture(1, 32000, 14.0, f0_hz=150.0, seed=23)
    for chunk in (0, 1000):
        o = orc.Oracle(orc.ARGOS, 32000, iq, chunk=chunk, sampler=1, math_mode=orc.MATH_LIBM)
        with pdt.Demodulator(pdt.MODE_ARGOS, 32000, chunk=chunk, sampler=pdt.SAMPLER_MM) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            assert d.stats().frames >= 5
    with pytest.raises(pdt.PdtError):
        pdt.Demodulator(pdt.MODE_POES, 50000, sampler=pdt.SAMPLER_MM, mm_step_range=1e9).demod(np.zeros((20000, 2), dtype=np.int16))


def test_cli_demodpoes(pdt, tmp_path):
    exe = os.path.join(ROOT, "bin", "demodPOES")
    out = tmp_path / "mf.txt"
    r = subprocess.run([exe, "-o", str(out), os.path.join(GOLDEN, "5sec_clip.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == golden_text("clip.c10000.txt")
    assert "Normalization Factor: 17.583342" in r.stdout
    assert " : PLL locked at -3466.19Hz" in r.stdout
    # no frames -> output file removed (POESTIPdemod/main.c:508-512)
    silent = tmp_path / "silence.wav"
    pdt.write_wav(str(silent), 50000, np.zeros((30000, 2), dtype=np.int16))
    out2 = tmp_path / "none.txt"
    r = subprocess.run([exe, "-o", str(out2), str(silent)], capture_output=True, text=True)
    assert r.returncode == 0 and not out2.exists()
    assert "None bits found" in r.stdout


def test_pass_shaped_snr_profile(pdt, orc):
    """A pass as a receiver sees it: 20 dB SNR in the middle, falling to about 0 dB at acquisition and loss of signal (noise
    scaled x10 at both ends, in steps).  The weak ends are where the block-parallel PLL stops merging and the seam repairs
    (region passes + final pass) carry the result: every stage equal to the oracle, and the repairs really ran."""
    import ctypes as C
    fs, seg_s = 50000, 6.0
    n = int(fs * seg_s)
    parts = []
    for k, mult in enumerate([10, 7, 4, 2, 1, 1, 2, 4, 7, 10]):
        p = pdt.synth_params(0, fs, 1000.0, 4711)
        p.noise_gain = int(p.noise_gain * mult)
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), k * n, n, iq.ctypes.data)          # one continuous signal, noise level per segment
        parts.append(iq)
    cap = np.concatenate(parts)
    o = orc.Oracle(orc.POES, fs, cap)
    os.environ["PDT_PLL_NOCONSENSUS"] = "1"           # (the walkers on their own: the repairs really run)
    try:
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(cap)
            check_all_stages(pdt, orc, d, o)
            s = d.stats()
            lone = s.pll_seam_fixes
            assert lone >= 10 and s.frames >= 400
    finally:
        del os.environ["PDT_PLL_NOCONSENSUS"]
    with pdt.Demodulator(pdt.MODE_POES, fs) as d:     # with the wavefronts' consensus (the default): fewer lost walkers, same result
        d.demod(cap)
        check_all_stages(pdt, orc, d, o)
        s = d.stats()
        assert s.pll_seam_fixes <= lone and s.frames >= 400


def test_fades_and_a_noise_tail_all_stages(pdt, orc):
    """Round 6, the tail pass (k_pll_tail_scan / k_pll_tail): stretches where the tracking loop has nothing to track -- two fades
    inside the signal, one of them leaving a little of it (patchy: blocks that merge between open seams), and a noise tail behind
    the loss of signal -- are walked from the last merged block in front of each, beside the acquisition.  Every stage equal to the
    oracle, with the tail pass and without it (PDT_PLL_NOTAIL: k_pll_fix alone), small PLL blocks so that the stretches span
    hundreds of seams; and the tail pass really took the repairs over."""
    import ctypes as C
    fs, seg_s = 50000, 3.0
    n = int(fs * seg_s)
    parts = []
    for k, amp in enumerate([1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.06, 0.06, 1.0, 1.0, 0.0, 0.0]):
        p = pdt.synth_params(0, fs, -1500.0, 4712)
        p.amplitude = int(round(p.amplitude * amp))
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), k * n, n, iq.ctypes.data)          # one continuous signal, amplitude per segment
        parts.append(iq)
    cap = np.concatenate(parts)
    o = orc.Oracle(orc.POES, fs, cap)
    fixes = {}
    for name, env in (("tail", {}), ("notail", {"PDT_PLL_NOTAIL": "1"})):
        os.environ.update(env)
        try:
            with pdt.Demodulator(pdt.MODE_POES, fs, pll_block=1024, profile=True) as d:
                d.demod(cap)
                check_all_stages(pdt, orc, d, o)
                fixes[name] = d.stats().pll_seam_fixes
                kt = d.kernel_times()
                assert ("pll_tail" in kt) == (name == "tail")
        finally:
            for k in env:
                os.environ.pop(k, None)
    assert fixes["tail"] >= 100 and fixes["notail"] >= 100, fixes      # (both count the walked blocks: the stretches are ~9 s of 36)
