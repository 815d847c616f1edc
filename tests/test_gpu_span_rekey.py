"""The staged span walk of the sampler's boundary-state tables: stage 1 walks the distinct exits of a row's first
chunk through a few chunks, k_gardner_span_rekey deduplicates the states they have merged into, stage 2 walks those -- several rows
to a wavefront -- through the rest of the row, k_gardner_span_spread hands every key its representative's records and tail.  No
float operation of a surviving trajectory changes, so every stage equals the ORACLE bit for bit, whatever the re-key point
(PDT_GSPAN_REKEY) and the lanes per row in stage 2 (PDT_GSPAN_SUB); rows are forced on short captures through PDT_GSPAN."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_parity import check_all_stages
from test_gpu_stream import stream_all

pytestmark = pytest.mark.gpu

_refs = {}


def capture(pdt, orc, fs, secs, chunk, seed):
    """A synthetic capture and its oracle, computed once and shared (never modified)."""
    key = (fs, secs, chunk, seed)
    if key not in _refs:
        iq = pdt.synth_capture(0, fs, secs, seed=seed)
        _refs[key] = (iq, orc.Oracle(orc.POES, fs, iq, chunk=chunk))
    return _refs[key]


def with_env(env, fn):
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def span_rekey(pdt, d):
    """pdt_dev_span_rekey: per row (keys behind the first chunk, distinct states at the re-key point, stage-2 items)."""
    L = pdt.lib()
    L.pdt_dev_span_rekey.restype = C.c_uint64
    L.pdt_dev_span_rekey.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    rows = int(L.pdt_dev_span_rekey(d._h, None, 0))
    out = np.zeros((rows, 3), dtype=np.uint32)
    if rows:
        assert int(L.pdt_dev_span_rekey(d._h, out.ctypes.data, rows)) == rows
    return out


CAPTURES = [(250000, 12.0, 0, 13), (250000, 12.0, 0, 3), (250000, 12.02, 0, 13), (250000, 9.0, 2500, 7), (50000, 30.0, 1000, 16),
            (250000, 12.0, 0, 20)]


@pytest.mark.parametrize("fs,secs,chunk,span", CAPTURES)
def test_every_stage_equals_the_oracle(pdt, orc, fs, secs, chunk, span):
    """Re-key points 1, 2, 3 and 8 or 16 lanes per row: a full row of 13, a row of 3 (re-key point 2 leaves stage 2 nothing: stage 1
    walks the rows through; 3 is past the row's end), a short last chunk, small chunks, 16 chunks of 1 000 samples, and a row of
    20 -- longer than the span rule chooses by itself."""
    iq, o = capture(pdt, orc, fs, secs, chunk, 300 + span)
    for a in (1, 2, 3):
        for sub in (8, 16):
            def run():
                with pdt.Demodulator(pdt.MODE_POES, fs, chunk=chunk) as d:
                    d.demod(iq)
                    check_all_stages(pdt, orc, d, o)
                    st = d.stats()
                    assert st.gardner_parallel == 1 and st.frames > 20
                    return span_rekey(pdt, d)
            info = with_env({"PDT_GSPAN": str(span), "PDT_GSPAN_REKEY": str(a), "PDT_GSPAN_SUB": str(sub)}, run)
            assert len(info) == (-(-len(iq) // (chunk or 10000)) - 1) // span, (a, sub)
            staged = a < span - 1
            assert bool(info[:, 1].any()) == staged and bool(info[:, 2].any()) == staged, (a, sub)
            if staged:
                assert (info[:, 1] <= info[:, 0]).all() and (info[:, 2] == -(-info[:, 1].astype(np.int64) // sub)).all(), (a, sub)


def test_rows_wider_than_a_sub_group(pdt, orc):
    """Eight lanes per row and more than eight states at the re-key point: the row takes a second item.  And the merge is real:
    in most rows fewer states go into stage 2 than keys went into stage 1."""
    iq, o = capture(pdt, orc, 250000, 12.0, 0, 313)

    def run():
        with pdt.Demodulator(pdt.MODE_POES, 250000) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            return span_rekey(pdt, d)
    info = with_env({"PDT_GSPAN": "13", "PDT_GSPAN_REKEY": "2", "PDT_GSPAN_SUB": "8"}, run)
    print("keys, states, items per row:", info.tolist())
    assert (info[:, 2] >= 2).any()
    assert 2 * int((info[:, 1] < info[:, 0]).sum()) > len(info)


@pytest.mark.parametrize("cap", [None, "2000"])
def test_noise_and_overflowing_key_lists(pdt, orc, cap):
    """Noise in front of the signal: the scouts list the whole domain, thousands of exits per row.  Such a row is not
    deduplicated -- stage 1 walks it through -- and with a key list too small for it (PDT_GSPAN_CAP) it is left untabulated and the
    chain walks it, as ever."""
    fs = 250000
    key = ("noise", fs)
    if key not in _refs:
        rng = np.random.default_rng(15)
        noise = np.clip(np.rint(rng.normal(0, 900, (int(1.0 * fs), 2))), -32768, 32767).astype("<i2")
        iq = np.ascontiguousarray(np.concatenate([noise, pdt.synth_capture(0, fs, 5.0, seed=48)]))
        _refs[key] = (iq, orc.Oracle(orc.POES, fs, iq))
    iq, o = _refs[key]
    env = {"PDT_GSPAN": "8", "PDT_GSPAN_REKEY": "2", "PDT_GSPAN_SUB": "8"}
    if cap:
        env["PDT_GSPAN_CAP"] = cap

    def run():
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            st = d.stats()
            assert st.gardner_parallel == 1 and st.gardner_full_domain > 0
            if cap:
                assert st.gardner_walked > 0
            return span_rekey(pdt, d)
    info = with_env(env, run)
    wide = (info[:, 0] > 256)                                 # (untabulated rows report 0xffffffff keys)
    assert wide.any() and not info[wide, 1].any() and not info[wide, 2].any()


def test_chain_takes_a_spread_tail(pdt, orc):
    """The chain walks the first chunk of a row it enters outside the scouts' band and takes the rest of the row from the
    recorded tail of the exit it finds -- with the staged walk a tail that k_gardner_span_spread wrote."""
    fs, secs = 250000, 24.0
    key = ("weak", fs)
    if key not in _refs:
        p = pdt.synth_params(0, fs, 1000.0, 91)
        p.noise_gain = int(p.noise_gain * 4)
        n = int(round(secs * fs))
        iq = np.zeros((n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, n, iq.ctypes.data)
        _refs[key] = (iq, orc.Oracle(orc.POES, fs, iq))
    iq, o = _refs[key]

    def run():
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            assert d.stats().gardner_walked > 0, "no row entered outside its band on this capture: the path was not exercised"
            assert span_rekey(pdt, d)[:, 1].any()
    with_env({"PDT_GSPAN": "4", "PDT_BAND_PAD": "0.002", "PDT_GSPAN_REKEY": "1"}, run)


def test_batch_of_two_captures(pdt, orc):
    """Two captures share the launches of a batch, each with its own lists and cursors."""
    import torch
    fs = 250000
    caps = [capture(pdt, orc, fs, 12.0, 0, 313), capture(pdt, orc, fs, 12.0, 0, 303)]

    def run():
        dev = [torch.from_numpy(iq.reshape(-1).copy()).to("cuda:0") for iq, _ in caps]
        torch.cuda.synchronize()
        ds = [pdt.Demodulator(pdt.MODE_POES, fs) for _ in caps]
        try:
            pdt.demod_batch(ds, [t.data_ptr() for t in dev], [len(iq) for iq, _ in caps])
            for d, (_, o) in zip(ds, caps):
                assert d.text() == o.text()
                assert span_rekey(pdt, d)[:, 1].any()
        finally:
            for d in ds:
                d.close()
    with_env({"PDT_GSPAN": "13", "PDT_GSPAN_REKEY": "2", "PDT_GSPAN_SUB": "8"}, run)


def test_stream_segment_with_rows(pdt, orc):
    """An aligned stream segment runs rows of several chunks (tests/test_gpu_stream.py, the whole-capture kernels): staged too, and
    its text is the one-shot result."""
    fs, block = 250000, 1040000
    iq = pdt.synth_capture(0, fs, 24.0, seed=71)

    def run():
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            d.demod(iq)
            want = d.text()
        with pdt.Demodulator(pdt.MODE_POES, fs) as d:
            got, _, _ = stream_all(d, iq, block)
            assert d.text() == want and pdt.format_frames(got) == want and len(got) >= 24 * 10 - 12
            assert span_rekey(pdt, d)[:, 1].any()            # (the last segment's rows)
    with_env({"PDT_GSPAN": "13", "PDT_GSPAN_REKEY": "2"}, run)


def test_single_stage_path_is_still_there(pdt, orc):
    """PDT_GSPAN_REKEY=0: one stage, as before round 20."""
    iq, o = capture(pdt, orc, 250000, 12.0, 0, 313)

    def run():
        with pdt.Demodulator(pdt.MODE_POES, 250000) as d:
            d.demod(iq)
            check_all_stages(pdt, orc, d, o)
            info = span_rekey(pdt, d)
            assert len(info) == 23 and info[:, 0].all() and not info[:, 1:].any()
    with_env({"PDT_GSPAN": "13", "PDT_GSPAN_REKEY": "0"}, run)
