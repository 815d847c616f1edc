"""bench.py's host-side rules (no GPU): what `roofline.bound` says for a kernel, from the evidence the line carries, and what
`--dump-outputs` writes."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_rules_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_roofline_bound_rule():
    b = load_bench()
    alg = 7_200_000_000
    # the bytes already move at >= 85 % of what streaming kernels reach: "hbm", whatever the issue counters say
    assert b.roofline_bound(5.33, 27_700_000_000, alg, 0.79) == "hbm"
    # the same kernel with less traffic per launch: the wavefronts issue in > 60 % of their cycles -> "issue"
    assert b.roofline_bound(5.44, 24_070_000_000, alg, 0.76) == "issue"
    # no SQ pass of this build committed: the traffic alone decides between "hbm" (more than half the time at that rate) and "latency"
    assert b.roofline_bound(5.44, 24_070_000_000, alg, None) == "hbm"
    assert b.roofline_bound(5.44, None, alg, None) == "latency"          # algorithmic bytes only: 1.3 TB/s
    assert b.roofline_bound(0.0, None, alg, None) == "latency"
    # a streaming kernel is "hbm" by its algorithmic bytes alone
    assert b.roofline_bound(1.28, None, alg, None) == "hbm"


def _frames(pdt, n, seed):
    rng = np.random.default_rng(seed)
    f = np.zeros(n, dtype=pdt.FRAME_DTYPE)
    f["time"] = np.sort(rng.random(n)) * 3600.0
    f["bit_index"] = np.sort(rng.integers(0, 1 << 40, n))
    f["time_src"] = rng.integers(0, 1 << 33, n)
    f["inverted"] = rng.integers(0, 2, n)
    f["nbytes"] = 104
    f["complete"] = rng.integers(0, 2, n)
    f["bytes"] = rng.integers(0, 256, (n, 104))
    return f


def test_dump_outputs_writes_every_frame_exactly(pdt, tmp_path):
    """--dump-outputs: the frame records of every capture, field by field in float32 / float64, and the result statistics."""
    b = load_bench()
    f0, f1 = _frames(pdt, 300, 1), _frames(pdt, 0, 2)
    s = pdt.Stats(samples=900, symbols=77, bits=66, frames=300, lock_sample=-1, lock_freq_hz=-3466.19, avg_phase=0.25)
    shapes = b.dump_outputs(str(tmp_path), [(0, f0, s), (1, f1, None)])
    got = {k: np.load(tmp_path / f"{k}.npy") for k in shapes}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["frames_capture"].tolist() == [0.0] * 300
    assert np.array_equal(got["frames_time"], f0["time"]) and np.array_equal(got["frames_bit_index"].astype(np.int64), f0["bit_index"])
    assert np.array_equal(got["frames_time_src"].astype(np.int64), f0["time_src"])
    for k in ("inverted", "nbytes", "complete"):
        assert np.array_equal(got[f"frames_{k}"].astype(np.uint8), f0[k])
    assert got["frames_bytes"].shape == (300, 104) and np.array_equal(got["frames_bytes"].astype(np.uint8), f0["bytes"])
    assert got["stats"].shape == (1, 1 + len(b.STATS_DUMPED))
    st = dict(zip(("capture",) + b.STATS_DUMPED, got["stats"][0]))
    assert st["capture"] == 0 and st["frames"] == 300 and st["lock_sample"] == -1 and st["lock_freq_hz"] == -3466.19


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(pdt, tmp_path):
    """Beyond the size limit the frames are a fixed, seeded sample (in order): two runs on the same frames write the same files."""
    b = load_bench()
    frames = [(r, _frames(pdt, 500, 10 + r), None) for r in range(3)]
    limit = 200 * 460
    a, c = tmp_path / "a", tmp_path / "c"
    b.dump_outputs(str(a), frames, limit=limit)
    b.dump_outputs(str(c), frames, limit=limit)
    total = sum(os.path.getsize(p) - 128 for p in a.iterdir())                 # (.npy header: 128 bytes)
    assert total <= limit
    for p in a.iterdir():
        assert (c / p.name).read_bytes() == p.read_bytes(), p.name
    cap = np.load(a / "frames_capture.npy")
    t = np.load(a / "frames_time.npy")
    assert 0 < len(cap) < 1500 and np.all(np.diff(cap) >= 0) and set(cap.tolist()) == {0.0, 1.0, 2.0}
    allt = np.concatenate([f["time"] for _, f, _ in frames])
    assert np.isin(t, allt).all()
