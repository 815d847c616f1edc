"""Real ARGOS IQ on the CPU (tests/real_captures.py): the reference's ARGOSdemod/packet.wav -- on which the ARGOS chain never
locks --, the 50 kHz clip through the ARGOS chain, the 32 kHz recording through the POES chain, and bursts over the recording's
noise.  First group: the oracle against the reference's own objects (oracle/_ref), every stage, skipped where they were not
built.  Second group: the oracle against the committed digests and texts those objects gave (tests/golden/make_golden.py),
which is what the GPU tests (tests/test_gpu_real_argos.py) stand on where oracle/_ref is absent."""
import hashlib
import os

import numpy as np
import pytest

import real_captures as rc
from conftest import GOLDEN, golden_text
from test_oracle_ref import REF_ARGOS, REF_POES, STAGES, compare_all, run_ref

have_ref = os.path.exists(REF_POES) and os.path.exists(REF_ARGOS)
needs_ref = pytest.mark.skipif(not have_ref, reason="oracle/_ref not built (make -C oracle ref)")

ROW_IDS = [rc.golden_name(*row) for row in rc.ROWS]


def capture_wav(pdt, tmp_path, name):
    rate, iq = rc.capture(name)
    if name == "packet":
        return rc.PACKET_WAV
    if name == "clip":
        return rc.CLIP_WAV
    wav = tmp_path / (name + ".wav")
    pdt.write_wav(str(wav), rate, iq)
    return str(wav)


def all_plus_zero(a):
    """every element the bit pattern of +0.0 (-0.0 fails)"""
    return a.tobytes() == bytes(a.nbytes)


# ------------------------------------------------------------------ the oracle against the reference's objects

@needs_ref
@pytest.mark.parametrize("name,mode,chunk", rc.ROWS, ids=ROW_IDS)
def test_oracle_equals_the_reference_objects(orc, pdt, tmp_path, name, mode, chunk):
    text, dump = run_ref(REF_ARGOS if mode == rc.ARGOS else REF_POES, capture_wav(pdt, tmp_path, name), tmp_path, ["-c", str(chunk)])
    o = rc.oracle(name, mode, chunk)
    for stage in ("pll", "fir", "agc", "sym", "symt", "bits", "bitt", "avg") + (("lock", "agcraw") if mode == rc.ARGOS else ()):
        assert os.path.exists(f"{dump}.{stage}"), stage              # compare_all skips a dump that is not there
    compare_all(o, dump)
    assert o.text() == text
    rc.check_table_row(o, name, mode, chunk)
    assert (len(text) > 0) == (rc.TABLE[(name, mode, chunk)][4] > 0)
    if mode == rc.ARGOS and name != "realnoise":
        # never locked: Squelch mutes every sample, the stream in front of it and the lock stream are alive
        assert all_plus_zero(np.fromfile(f"{dump}.agc", dtype="<f8"))
        assert np.fromfile(f"{dump}.agcraw", dtype="<f8").any()
        assert np.fromfile(f"{dump}.lock", dtype="<f8").all()


@needs_ref
@pytest.mark.parametrize("name,mode,chunk", [r for r in rc.ROWS if r[1] == rc.ARGOS], ids=[i for i in ROW_IDS if i.startswith("argos")])
def test_portable_math_keeps_the_reference_output_on_real_input(orc, pdt, tmp_path, name, mode, chunk):
    """what test_argos_portable_math_keeps_the_reference_output claims for synthetic captures: with the plain-IEEE sine/cosine the
    symbols' pick indices, the bits and the packet file stay the reference's"""
    text, dump = run_ref(REF_ARGOS, capture_wav(pdt, tmp_path, name), tmp_path, ["-c", str(chunk)])
    rate, iq = rc.capture(name)
    o = orc.Oracle(orc.ARGOS, rate, iq, chunk=chunk, math_mode=orc.MATH_PORTABLE)
    assert o.text() == text
    assert o.stage(orc.ST_BITS).tobytes() == open(f"{dump}.bits", "rb").read()
    assert np.array_equal(o.stage(orc.ST_SYMIDX), rc.oracle(name, mode, chunk).stage(orc.ST_SYMIDX))
    ref_sym = np.fromfile(f"{dump}.sym", dtype=np.float64)
    sym = o.stage(orc.ST_SYM)
    assert len(sym) == len(ref_sym) == rc.TABLE[(name, mode, chunk)][2]
    assert np.allclose(sym, ref_sym, rtol=1e-9, atol=1e-12)          # same picks, last-bit differences only


# ------------------------------------------------------------------ the oracle against the committed digests and texts

def test_input_digests(golden):
    assert os.path.getsize(rc.PACKET_WAV) == 105816
    assert hashlib.sha256(open(rc.PACKET_WAV, "rb").read()).hexdigest() == golden["synth"][rc.PACKET_SHA256_KEY]
    rate, mix = rc.capture("realnoise")
    assert rate == 32000 and mix.shape == (416000, 2) and mix.dtype == np.dtype("<i2")
    assert hashlib.sha256(mix.tobytes()).hexdigest() == golden["synth"][rc.REALNOISE_SHA256_KEY]
    assert int(np.abs(mix.astype(np.int32)).max()) <= 2187 + 2754


def check_against_golden(o, golden, name, mode, chunk):
    """every committed digest of a row, its console lines and its text against an oracle-shaped object"""
    key = rc.golden_name(name, mode, chunk)
    for stage, digest in golden["stages"][key].items():
        assert hashlib.sha256(o.stage(STAGES[stage]).tobytes()).hexdigest() == digest, f"{key}: stage {stage} differs from the reference's dump"
    console = golden["console"][key]
    assert console[0] == f"Normalization Factor: {o.norm_factor:f}"
    if o.lock_sample >= 0:
        assert console[1:] == [f" : PLL locked at {o.lock_freq_hz:0.2f}Hz"]
    else:
        assert console[1:] == []
    path = os.path.join(GOLDEN, key + ".txt")
    assert o.text() == (golden_text(key + ".txt") if os.path.exists(path) else b"")


@pytest.mark.parametrize("name,mode,chunk", rc.ROWS, ids=ROW_IDS)
def test_oracle_equals_the_committed_reference_results(orc, golden, name, mode, chunk):
    o = rc.oracle(name, mode, chunk)
    key = rc.golden_name(name, mode, chunk)
    want = {"pll", "fir", "agc", "sym", "symt", "bits", "bitt", "avg"} | ({"lock", "agcraw"} if mode == rc.ARGOS else set())
    assert set(golden["stages"][key]) == want
    check_against_golden(o, golden, name, mode, chunk)
    rc.check_table_row(o, name, mode, chunk)
    if mode == rc.ARGOS and name != "realnoise":
        assert all_plus_zero(o.stage(orc.ST_AGC)) and o.stage(orc.ST_AGC_RAW).any() and o.stage(orc.ST_LOCK).all()
        assert all_plus_zero(o.stage(orc.ST_SYM))                    # the sampler walked +0.0 only
    if name == "realnoise":
        assert len(o.text()) == rc.TEXT_BYTES[chunk]
    if name == "packet" and mode == rc.ARGOS:
        avg = o.stage(orc.ST_AVG)
        assert len(avg) == rc.AVG_VALUES[chunk]
        if chunk != 2401:
            assert avg.tobytes() == golden_text(f"{key}.avg.f64")


def test_chunk_size_is_observable_on_real_noise():
    a, b = golden_text("argos_realnoise.c2400.txt"), golden_text("argos_realnoise.c2401.txt")
    assert (a.count(b"\n"), b.count(b"\n")) == (8, 7) and (len(a), len(b)) == (242, 212)


def test_default_chunk_is_the_tables_row(orc):
    """chunk 0 = the programs' defaults (2400 / 10000): the rows the GPU tests run with the default as well"""
    for name, mode, chunk in (("packet", rc.ARGOS, 2400), ("packet", rc.POES, 10000), ("clip", rc.ARGOS, 2400), ("realnoise", rc.ARGOS, 2400)):
        o0, o = rc.oracle(name, mode, 0), rc.oracle(name, mode, chunk)
        assert o0.text() == o.text() and o0.totals() == o.totals() and o0.norm_factor == o.norm_factor
        assert o0.stage(orc.ST_SYM).tobytes() == o.stage(orc.ST_SYM).tobytes()
