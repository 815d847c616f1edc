"""The oracle's restatement against the reference's own compiled objects (oracle/_ref) on silence, full scale, NaN and infinity: every
case of tests/degenerate_cases.py the reference's programs can take -- int16 through a WAV, float32 through a RAW file with -s (the
live chain: -L), ARGOS the int16 cases only -- every stage the dump holds and the text, under the rule of degenerate_cases (every NaN
one value, everything else byte for byte).  This pins the oracle on these inputs; tests/test_gpu_degenerate.py compares the kernels
with it.  Skipped where oracle/_ref was not built, as tests/test_oracle_ref.py is."""
import os

import numpy as np
import pytest

import degenerate_cases as dc
from test_oracle_ref import REF_ARGOS, REF_POES, STAGES, run_ref

pytestmark = pytest.mark.skipif(not (os.path.exists(REF_POES) and os.path.exists(REF_ARGOS)),
                                reason="oracle/_ref not built (make -C oracle ref)")


@pytest.mark.parametrize("name", [c[0] for c in dc.cases()])
def test_restatement_equals_the_reference_objects(orc, pdt, tmp_path, name):
    _, mode, fs, chunk, chain, a, expect = dc.case(name)
    o = dc.oracle(name)                                   # (asserts the case's own property first)
    extra = ["-c", str(chunk)] if chunk else []
    if a.dtype.kind == "f":
        path = tmp_path / "cap.raw"
        a.tofile(path)
        extra = (["-L"] if chain else []) + ["-s", repr(fs / 1000.0)] + extra
    else:
        assert not chain
        path = tmp_path / "cap.wav"
        pdt.write_wav(str(path), fs, a)
    text, dump = run_ref(REF_ARGOS if mode == dc.ARGOS else REF_POES, path, tmp_path, extra)
    compared = 0
    for stage, sid in STAGES.items():
        f = f"{dump}.{stage}"
        if not os.path.exists(f) or (stage == "lock" and mode == dc.POES and not chain):
            continue
        want = o.stage(sid)
        if stage == "iq":
            # the echo of the input, no stage of the chain: the reference forms realVal + imagVal * I (wave.c:166, :524), whose real
            # part is realVal + imagVal * 0 -- a NaN where the imaginary part is infinite or a NaN -- and the restatement keeps the
            # pair as read.  Its PLL gives both the same output (the pll stage above says so): the reference's complex multiply
            # takes (NaN, inf) for the infinity it is (C99 Annex G), the restatement's plain products never see the NaN
            want = want.reshape(-1, 2).copy()
            with np.errstate(invalid="ignore"):
                want[:, 0] += want[:, 1] * want.dtype.type(0)
            want = want.reshape(-1)
        raw = open(f, "rb").read()
        assert len(raw) == want.nbytes, f"stage {stage}: {len(raw)} bytes from the reference objects, {want.nbytes} from the restatement"
        dc.assert_stream_equal(stage, want, np.frombuffer(raw, dtype=want.dtype))
        compared += 1
    assert compared >= 9
    assert o.text() == text
    if expect.get("min_frames"):
        assert len(text) > 0


def test_fir_model_is_the_restatements_filter(orc):
    """degenerate_cases.fir_interp_model, the reference of the stage-level filter test on +inf and -inf, gives the oracle's FIR stream
    bit for bit (the first 1 500 inputs of a capture: 4 500 outputs from a zeroed ring)"""
    o = dc.oracle("p50-zero-3000")
    got = dc.fir_interp_model(o.stage(orc.ST_PLL)[:1500], o.stage(orc.ST_TAPS), o.interp)
    assert o.interp == 3 and got.tobytes() == o.stage(orc.ST_FIR)[:4500].tobytes()
