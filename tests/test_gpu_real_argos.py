"""Real ARGOS IQ through every entry point of the HIP path, bit for bit against the oracle (MATH_LIBM, which
tests/test_real_argos.py ties to the reference's own objects on these very inputs) and, where they exist, against the committed
results of those objects (tests/golden/make_golden.py).  The inputs are tests/real_captures.py's:

packet    : the reference's one real ARGOS recording.  The ARGOS chain never locks on it, so every seam is open, Squelch mutes
            every chunk, the sampler only adds its step (k_chunk_need, k_gardner_ring's one-stride path from the first sample to
            the last) and the time axis alone decides how many symbols come out.  Through the POES chain (the wrong mode): the
            5x interpolator on real data.
clip      : the 50 kHz NOAA-15 clip through the ARGOS chain (the wrong mode the other way): a sampler step of 62.5.
realnoise : synthetic bursts over the recording's noise: the post-Squelch stages on a real front end's noise; the number of
            packets depends on the chunk size (8 at 2400, 7 at 2401).
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch        # before libpdt is loaded (as in test_gpu_batch.py): torch brings its own HIP runtime

import real_captures as rc
from conftest import ROOT, golden_text
from test_gpu_batch import to_dev
from test_gpu_live import STAGES as TWIN_STAGES
from test_gpu_parity import assert_stage_equal, check_all_stages
from test_gpu_quality import check_reports
from test_gpu_stages import argos_agc_streams, chunks_of, gardner_replay, manchester_replay, pll_replay
from test_gpu_stream import stream_all

pytestmark = pytest.mark.gpu

ROW_IDS = [rc.golden_name(*row) for row in rc.ROWS]
DEFAULTS = [("packet", rc.ARGOS, 0), ("packet", rc.POES, 0), ("clip", rc.ARGOS, 0), ("realnoise", rc.ARGOS, 0)]
DEFAULT_CHUNK = {rc.ARGOS: 2400, rc.POES: 10000}


def all_plus_zero(a):
    """every element the bit pattern of +0.0 (-0.0 fails)"""
    return a.tobytes() == bytes(a.nbytes)


def norm_of(d):
    """the normalization factor as the chain's DECIMAL_TYPE holds it (double for ARGOS, float for POES)"""
    s = d.stats()
    return s.norm_factor if d.dtype == np.float64 else float(np.float32(s.norm_factor))


def check_golden_digests(pdt, d, golden, key):
    """the streams the context keeps against the digests of the reference objects' dumps"""
    ids = {"pll": pdt.ST_PLL, "lock": pdt.ST_LOCK, "fir": pdt.ST_FIR, "agc": pdt.ST_AGC, "agcraw": pdt.ST_AGC_RAW, "sym": pdt.ST_SYM,
           "bits": pdt.ST_BITS}
    for stage, digest in golden["stages"][key].items():
        if stage in ids:
            assert hashlib.sha256(d.stage(ids[stage]).tobytes()).hexdigest() == digest, f"{key}: stage {stage} differs from the reference's dump"
    rep = d.chunk_reports()
    dt = "<f8" if d.mode == pdt.MODE_ARGOS else "<f4"
    assert hashlib.sha256(rep["avg_phase"].astype(dt).tobytes()).hexdigest() == golden["stages"][key]["avg"]
    s = d.stats()
    console = golden["console"][key]
    assert console[0] == f"Normalization Factor: {norm_of(d):f}"
    assert console[1:] == ([f" : PLL locked at {s.lock_freq_hz:0.2f}Hz"] if s.lock_sample >= 0 else [])


def check_table(d, name, mode, chunk):
    lock, freq, nsym, nbits, nframes, norm = rc.TABLE[(name, mode, chunk)]
    s = d.stats()
    assert (s.samples, s.symbols, s.bits, s.frames) == (len(rc.capture(name)[1]), nsym, nbits, nframes)
    assert s.lock_sample == lock
    if freq is not None:
        assert f"{s.lock_freq_hz:0.2f}" == freq
    if norm is not None:
        assert f"{norm_of(d):f}" == norm


# ------------------------------------------------------------------ the one-shot chain

@pytest.mark.parametrize("name,mode,chunk", rc.ROWS + DEFAULTS, ids=ROW_IDS + [rc.golden_name(*r) for r in DEFAULTS])
def test_one_shot_chain(pdt, orc, golden, name, mode, chunk):
    rate, iq = rc.capture(name)
    o = rc.oracle(name, mode, chunk)
    row = (name, mode, chunk or DEFAULT_CHUNK[mode])
    key = rc.golden_name(*row)
    with pdt.Demodulator(mode, rate, chunk=chunk) as d:
        d.keep_quality()
        if mode == rc.ARGOS:
            d.keep_presquelch()
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        check_table(d, *row)
        avg = o.stage(orc.ST_AVG)
        check_reports(d.chunk_reports(), avg, None, "<f8" if mode == rc.ARGOS else "<f4")
        if mode == rc.ARGOS:
            assert_stage_equal("agcraw", d.stage(pdt.ST_AGC_RAW), o.stage(orc.ST_AGC_RAW))
            if name == "packet" and row[2] in (2400, 1000):
                check_reports(d.chunk_reports(), np.frombuffer(golden_text(f"{key}.avg.f64"), dtype="<f8"), None, "<f8")
        check_golden_digests(pdt, d, golden, key)
        if rc.TABLE[row][4] == 0:
            assert d.stats().frames == 0 and d.text() == b""
        if mode == rc.ARGOS and name != "realnoise":
            # never locked: Squelch mutes every sample; what stands in front of it, and the lock stream, are alive
            assert all_plus_zero(d.stage(pdt.ST_AGC)) and len(d.stage(pdt.ST_AGC)) == len(iq)
            assert d.stage(pdt.ST_AGC_RAW).any() and d.stage(pdt.ST_LOCK).all()
        if name == "realnoise":
            assert d.text() == golden_text(f"{key}.txt") and len(d.text()) == rc.TEXT_BYTES[row[2]]


# ------------------------------------------------------------------ the sampler's stride on a capture that is squelched from end to end

@pytest.mark.parametrize("name", ["packet", "clip"])
@pytest.mark.parametrize("chunk", [2400, 2401, 1999, 777])
def test_sampler_stride_on_an_all_squelched_capture(pdt, orc, name, chunk):
    """test_argos_squelched_chunks_in_one_stride on input where no burst guarantees a symbol: only the time axis provides them
    (662 from the recording, 4 004 from the clip, whatever the chunk size), with the stride and with it switched off."""
    rate, iq = rc.capture(name)
    o = rc.oracle(name, rc.ARGOS, chunk)
    for env in ({}, {"PDT_GARDNER_NOSTRIDE": "1"}):
        os.environ.update(env)
        try:
            with pdt.Demodulator(pdt.MODE_ARGOS, rate, chunk=chunk) as d:
                d.demod(iq)
                check_all_stages(pdt, orc, d, o)
                s = d.stats()
                assert (s.symbols, s.bits, s.frames) == ({"packet": 662, "clip": 4004}[name], {"packet": 331, "clip": 2002}[name], 0)
                assert s.lock_sample == -1 and all_plus_zero(d.stage(pdt.ST_AGC)) and all_plus_zero(d.stage(pdt.ST_SYM))
        finally:
            for k in env:
                os.environ.pop(k, None)


# ------------------------------------------------------------------ block geometry

@pytest.mark.parametrize("name,mode,kw", [
    ("packet", rc.ARGOS, dict(pll_block=256, pll_warm=256, agc_block=256, agc_warm=256)),
    ("packet", rc.ARGOS, dict(pll_block=1 << 30, pll_warm=0, agc_block=1 << 30, agc_warm=0)),
    ("realnoise", rc.ARGOS, dict(pll_block=256, pll_warm=256, agc_block=256, agc_warm=256)),
    ("realnoise", rc.ARGOS, dict(pll_block=1 << 30, pll_warm=0, agc_block=1 << 30, agc_warm=0)),
    ("packet", rc.POES, dict(pll_block=64, pll_warm=64, agc_block=64, agc_warm=64)),
], ids=["packet-256", "packet-one", "realnoise-256", "realnoise-one", "packet-poes-64"])
def test_block_geometry_never_changes_the_result(pdt, orc, name, mode, kw):
    rate, iq = rc.capture(name)
    o = rc.oracle(name, mode, 0)
    with pdt.Demodulator(mode, rate, **kw) as d:
        if mode == rc.ARGOS:
            d.keep_presquelch()
        d.demod(iq)
        check_all_stages(pdt, orc, d, o)
        check_table(d, name, mode, DEFAULT_CHUNK[mode])
        if mode == rc.ARGOS:
            assert_stage_equal("agcraw", d.stage(pdt.ST_AGC_RAW), o.stage(orc.ST_AGC_RAW))
        if kw["pll_block"] == 64:
            assert d.stats().pll_seam_fixes > 0 and d.stats().agc_seam_fixes > 0


# ------------------------------------------------------------------ short and ragged cuts of the real recording

@pytest.mark.parametrize("k", [0, 10007])
@pytest.mark.parametrize("n", [0, 1, 3, 2399, 2400, 2401, 4800])
def test_short_and_ragged_cuts(pdt, orc, k, n):
    """empty, less than one chunk, a chunk exactly, one sample more, two chunks; the cuts at 10 007 lock (sample 1 266) and still
    carry no packet, the cuts at 0 do not lock"""
    rate, iq = rc.capture("packet")
    part = iq[k:k + n]
    o = orc.Oracle(orc.ARGOS, rate, part, math_mode=orc.MATH_LIBM)
    with pdt.Demodulator(pdt.MODE_ARGOS, rate) as d:
        d.keep_presquelch().demod(part)
        check_all_stages(pdt, orc, d, o)
        assert_stage_equal("agcraw", d.stage(pdt.ST_AGC_RAW), o.stage(orc.ST_AGC_RAW))
        assert d.stats().frames == 0
        assert d.stats().lock_sample == (1266 if k and n >= 2399 else -1)


# ------------------------------------------------------------------ the alternative kernels

@pytest.mark.parametrize("switch", ["PDT_FIR_GENERIC", "PDT_AGC_UNFUSED", "PDT_GARDNER_ONEBUF", "PDT_GARDNER_NORING", "PDT_EMA_NOGUESS",
                                    "PDT_GARDNER_SEQUENTIAL", "PDT_AGC_LANES"])
def test_alternative_kernels_agree_on_real_input(pdt, orc, switch):
    """the switches of test_alternative_kernels_agree, on the recording through the POES chain and on bursts over its noise"""
    os.environ[switch] = "1"
    try:
        for name, mode in (("packet", rc.POES), ("realnoise", rc.ARGOS)):
            rate, iq = rc.capture(name)
            with pdt.Demodulator(mode, rate) as d:
                d.demod(iq)
                check_all_stages(pdt, orc, d, rc.oracle(name, mode, 0))
                check_table(d, name, mode, DEFAULT_CHUNK[mode])
    finally:
        del os.environ[switch]


# ------------------------------------------------------------------ the stage entry points

@pytest.mark.parametrize("chunk", [2400, 1001])
def test_pll_stage_from_pcm16(pdt, orc, chunk):
    """CarrierTrackPLL (double build) chunk after chunk on the recording: realDataOut, the lock stream, the return values (the
    reference's own at 2400), and a lock that never happens"""
    rate, iq = rc.capture("packet")
    o = rc.oracle("packet", rc.ARGOS, chunk)
    with pdt.Demodulator(pdt.MODE_ARGOS, rate, chunk=chunk) as d:
        out, lock, rets, st = pll_replay(pdt, d, iq, chunk)
        assert_stage_equal("pll", out, o.stage(orc.ST_PLL))
        assert_stage_equal("lock", lock, o.stage(orc.ST_LOCK))
        avg = o.stage(orc.ST_AVG)
        assert len(rets) == -(-len(iq) // chunk) and rets.tobytes() == avg[:len(rets)].tobytes()
        if chunk == 2400:
            assert rets.astype("<f8").tobytes() == golden_text("argos_packet.c2400.avg.f64")
        assert st.started == 1 and st.locked == 0 and lock.all()
        out2, lock2, _, st2 = pll_replay(pdt, d, iq, 50000)                # any other cut of the same stream
        assert out2.tobytes() == out.tobytes() and lock2.tobytes() == lock.tobytes()
        for f in ("phase", "freq", "avg_phase", "locksig", "sweep"):
            assert getattr(st, f) == getattr(st2, f), f


@pytest.mark.parametrize("mode,chunk", [(rc.ARGOS, 2400), (rc.POES, 10000), (rc.POES, 777)], ids=["argos", "poes-x5", "poes-x5-777"])
def test_fir_stage(pdt, orc, mode, chunk):
    """LowPassFilter (ARGOS, 50 taps, double) and LowPassFilterInterp (POES at 32 kHz: x5, 130 taps) on the recording's PLL stream"""
    rate, _ = rc.capture("packet")
    o = rc.oracle("packet", mode, chunk)
    x, want = o.stage(orc.ST_PLL), o.stage(orc.ST_FIR)
    assert len(want) == len(x) * (5 if mode == rc.POES else 1)
    with pdt.Demodulator(mode, rate, chunk=chunk) as d:
        st = pdt.FirState()
        got = np.concatenate([d.stage_fir(x[a:b], st) for a, b in chunks_of(len(x), chunk)])
        assert got.dtype == want.dtype
        assert_stage_equal("fir", got, want)
        assert st.count == len(x)


@pytest.mark.parametrize("name,chunk", [("packet", 2400), ("packet", 2401), ("realnoise", 2400)])
def test_agc_and_squelch_stages(pdt, orc, name, chunk):
    norm_factor, (x, raw, want, lock) = argos_agc_streams(pdt, orc, name, chunk)
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000, chunk=chunk) as d:
        st = pdt.AgcState()
        got = np.concatenate([d.stage_agc(x[a:b], norm_factor, st) for a, b in chunks_of(len(x), chunk)])
        assert_stage_equal("agcraw", got, raw)                                  # NormalizingAGC alone: what -r dumps
        sq = np.concatenate([d.stage_squelch(got[a:b], lock[a:b], 0.15) for a, b in chunks_of(len(x), chunk)])
        assert_stage_equal("agc", sq, want)                                     # ... then Squelch (ARGOSdemod/main.c:276)
        assert all_plus_zero(sq) == (name == "packet") and got.any()


@pytest.mark.parametrize("name,chunk", [("packet", 2400), ("packet", 2401), ("realnoise", 2400), ("realnoise", 2401)])
def test_gardner_manchester_and_bytesync_stages(pdt, orc, name, chunk):
    """GardenerClockRecovery with the reads past the buffer landing in the lock-signal array behind it (Q16), both alignments of
    the heap's size field: on a stream of +0.0 only (the recording: the lock stream behind it is NOT zero) and on bursts over real
    noise; then ManchesterDecode on those symbols, and the synchroniser on realnoise's bits"""
    o = rc.oracle(name, rc.ARGOS, chunk)
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000, chunk=chunk) as d:
        sym, pick, _ = gardner_replay(pdt, d, o.stage(orc.ST_AGC), chunk, lock=o.stage(orc.ST_LOCK))
        assert_stage_equal("sym", sym, o.stage(orc.ST_SYM))
        assert np.array_equal(pick, o.stage(orc.ST_SYMIDX))
        bits, bsym, _ = manchester_replay(pdt, d, o.stage(orc.ST_SYM), o.stage(orc.ST_SYMIDX), chunk, 0.5)
        assert bits.tobytes() == o.stage(orc.ST_BITS).tobytes() and len(bits) == rc.TABLE[(name, rc.ARGOS, chunk)][3]
        assert o.stage(orc.ST_SYMT)[bsym].tobytes() == o.stage(orc.ST_BITT).tobytes()
    if name == "realnoise":
        text, frames = orc.bytesync(orc.ARGOS, o.stage(orc.ST_BITS))
        with pdt.Demodulator(pdt.MODE_ARGOS, 32000) as d:
            d.bytesync(o.stage(orc.ST_BITS))
            got = d.frames_array()
            assert d.text() == text and len(got) == len(frames) >= 7
            for g, f in zip(got, frames):
                assert (g["time"], g["bit_index"], g["inverted"], g["nbytes"], g["complete"]) == f[:5] and bytes(g["bytes"]) == f[5]


# ------------------------------------------------------------------ batch

def test_batch_of_real_captures(pdt, orc):
    """one pdt_demod_batch_device call: the recording as ARGOS and as POES, bursts over its noise, the clip as ARGOS at 50 kHz and
    an empty capture; every slot equals its own oracle, and again on the same contexts"""
    slots = [("packet", rc.ARGOS), ("packet", rc.POES), ("realnoise", rc.ARGOS), ("clip", rc.ARGOS)]
    caps = [rc.capture(name)[1] for name, _ in slots] + [np.zeros((0, 2), dtype=np.int16)]
    oracles = [rc.oracle(name, mode, 0) for name, mode in slots] + [orc.Oracle(orc.ARGOS, 32000, caps[-1], math_mode=orc.MATH_LIBM)]
    dev = [to_dev(iq) for iq in caps]
    torch.cuda.synchronize()
    ds = [pdt.Demodulator(mode, rc.capture(name)[0]) for name, mode in slots] + [pdt.Demodulator(pdt.MODE_ARGOS, 32000)]
    try:
        for rep in range(2):
            pdt.demod_batch(ds, [t.data_ptr() for t in dev], [len(iq) for iq in caps])
            for d, o in zip(ds, oracles):
                check_all_stages(pdt, orc, d, o)
            for d, (name, mode) in zip(ds, slots):
                check_table(d, name, mode, DEFAULT_CHUNK[mode])
    finally:
        for d in ds:
            d.close()


# ------------------------------------------------------------------ streaming

@pytest.mark.parametrize("name", ["packet", "realnoise"])
@pytest.mark.parametrize("block", [2400, 2401, 777])
def test_stream_in_blocks(pdt, orc, name, block):
    """pdt_stream_* pushes: the frames of the one-shot chain, once and in order, and its counters (what
    test_stream_against_the_oracle asserts for the clip)"""
    rate, iq = rc.capture(name)
    o = rc.oracle(name, rc.ARGOS, 0)
    with pdt.Demodulator(pdt.MODE_ARGOS, rate) as d:
        got, _, _ = stream_all(d, iq, block)
        assert pdt.format_frames(got) == o.text() == d.text()
        assert got.tobytes() == d.frames_array().tobytes()
        check_table(d, name, rc.ARGOS, 2400)
        s = d.stats()
        assert s.lock_sample == o.lock_sample and s.norm_factor == o.norm_factor
        if o.lock_sample >= 0:
            assert f"{s.lock_freq_hz:0.2f}" == f"{o.lock_freq_hz:0.2f}"
        if name == "realnoise":
            assert d.text() == golden_text("argos_realnoise.c2400.txt")


# ------------------------------------------------------------------ the sound-card twin

@pytest.mark.parametrize("name", ["packet", "realnoise"])
def test_argos_twin_on_real_input(pdt, orc, tmp_path, name):
    """mode ARGOS + chain LIVE (the float build of the ARGOS chain) on the captures as float32, every stage against the oracle
    and, where the reference's float objects travelled with the tree, the text against theirs"""
    rate, iq = rc.capture(name)
    o = rc.oracle(name, rc.ARGOS, 0, chain=1)
    with pdt.Demodulator(pdt.MODE_ARGOS, rate, chain=pdt.CHAIN_LIVE) as d:
        assert d.dtype == np.float32
        d.demod_raw(rc.as_float(iq))
        for st in TWIN_STAGES:
            got, exp = d.stage(getattr(pdt, st)), o.stage(getattr(orc, st))
            assert got.dtype == exp.dtype
            assert_stage_equal(st, got, exp)
        assert d.text() == o.text()
        s = d.stats()
        ns, nsym, nbits, nfr = o.totals()
        assert (s.samples, s.symbols, s.bits, s.frames) == (ns, nsym, nbits, nfr) == (len(iq),) + rc.TABLE[(name, rc.ARGOS, 2400)][2:5]
        assert s.lock_sample == o.lock_sample == rc.TABLE[(name, rc.ARGOS, 2400)][0]
        if name == "packet":
            assert all_plus_zero(d.stage(pdt.ST_AGC))
        exe = os.path.join(ROOT, "oracle", "_ref", "ref_demodARGOSf")
        if os.path.exists(exe):
            wav, out = tmp_path / "a.wav", tmp_path / "ref.txt"
            pdt.write_wav(str(wav), rate, iq)
            subprocess.run([exe, str(wav), str(out)], check=True, capture_output=True)
            assert d.text() == (out.read_bytes() if out.exists() else b"")


# ------------------------------------------------------------------ the reference's chunk loop over the shim

@pytest.mark.parametrize("chunk", [2400, 2401])
def test_shim_on_real_input(pdt, tmp_path, chunk):
    """oracle/_ref/compat_demodARGOS (test_shim_argos's harness): no packet file for the recording, the reference's for realnoise"""
    exe = os.path.join(ROOT, "oracle", "_ref", "compat_demodARGOS")
    if not os.path.exists(exe):
        pytest.skip("compat_demodARGOS not built (needs the reference tree at build time)")
    out = tmp_path / "pk.txt"
    r = subprocess.run([exe, "-c", str(chunk), rc.PACKET_WAV, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not out.exists()
    assert f"Normalization Factor: {rc.TABLE[('packet', rc.ARGOS, chunk)][5]}" in r.stdout and "locked" not in r.stdout
    wav = tmp_path / "realnoise.wav"
    pdt.write_wav(str(wav), 32000, rc.capture("realnoise")[1])
    r = subprocess.run([exe, "-c", str(chunk), str(wav), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert out.read_bytes() == golden_text(f"argos_realnoise.c{chunk}.txt")


# ------------------------------------------------------------------ the host programs

def test_cli_on_the_real_recording(pdt, orc, golden, tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([os.path.join(ROOT, "bin", "demodARGOS"), "-o", str(out), rc.PACKET_WAV], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    console = golden["console"]["argos_packet.c2400"]
    assert console == ["Normalization Factor: 17.731425"]
    assert [l for l in r.stdout.splitlines() if "Normalization" in l] == console and "locked" not in r.stdout
    assert not out.exists()                                  # no packets: the reference removes the file (ARGOSdemod/main.c:320)
    assert not (tmp_path / "output.raw").exists()
    r = subprocess.run([os.path.join(ROOT, "bin", "demodARGOS"), "-r", "-o", str(out), rc.PACKET_WAV], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    want = rc.oracle("packet", rc.ARGOS, 0).stage(orc.ST_AGC_RAW)
    assert len(want) == 26443 and (tmp_path / "output.raw").read_bytes() == want.tobytes()
    assert not out.exists()
    out2 = tmp_path / "mf.txt"
    r = subprocess.run([os.path.join(ROOT, "bin", "demodPOES"), "-o", str(out2), rc.PACKET_WAV], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert " : PLL locked at -492.04Hz" in r.stdout
    assert [l for l in r.stdout.splitlines() if "Normalization" in l] == golden["console"]["poes_packet.c10000"][:1]
    assert not out2.exists()
