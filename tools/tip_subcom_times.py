#!/usr/bin/env python3
"""The subcommutation kernels' times: k_subcom_mark, k_subcom_count, k_subcom_scan, k_subcom_place and k_subcom_spikes from
a profiled context's pdt_kernel_times, the wall time of pdt_tip_subcom_records and the wall time of pdt_host_tip_subcom on the same
records, under the SEM table, the housekeeping table and a table of 256 entries, on two sets of records: the minor frames
`bench.py --config pass`'s capture transmits while its signal is up (60 s .. 840 s: 7 800 frames of kind 0) and 36 000 frames of kind 4,
an hour.  The records are built from the synthesiser's frames, not demodulated.

    python tools/tip_subcom_times.py --out profiles/r28/tip_subcom_times.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def records(pdt, p, first, count):
    fr = np.zeros(count, dtype=pdt.FRAME_DTYPE)
    for k in range(count):
        fr["bytes"][k] = pdt.synth_poes_frame(p, first + k)
    fr["bit_index"] = 18 + 832 * np.arange(count)
    fr["time"] = (first + np.arange(count)) * 0.1
    fr["nbytes"], fr["complete"] = 104, 1
    return fr


def wide_table(pdt):
    """256 entries, two a channel: periods 1 .. 320, bytes all over the frame (48 samples a record)"""
    rng = np.random.default_rng(5)
    t = np.zeros(256, dtype=pdt.SUBCOM_ENTRY_DTYPE)
    for k in range(256):
        period = int(rng.choice([1, 2, 4, 5, 8, 10, 16, 20, 32, 40, 64, 80, 160, 320]))
        t[k] = (k % 128, int(rng.integers(0, 104)), period, int(rng.integers(0, period)), 0xFF, 0, 0, 0)
    return t


def measure(pdt, d, fr, table, reps):
    cap = 1 << 21
    d.tip_subcom_records(fr, table, cap=cap)                             # (the first call allocates the work buffer)
    wall, kernels = [], {}
    for _ in range(reps):
        t0 = time.perf_counter()
        got = d.tip_subcom_records(fr, table, cap=cap)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k, (launches, ms) in d.kernel_times().items():
            if k.startswith("k_subcom_"):
                kernels.setdefault(k, []).append(ms)
    host = []
    for _ in range(max(3, reps // 4)):
        t0 = time.perf_counter()
        want = pdt.host_tip_subcom(fr, table, cap=cap)
        host.append((time.perf_counter() - t0) * 1e3)
    assert got[1] == want[1] and got[3] == want[3] and got[2].tobytes() == want[2].tobytes() and got[0].tobytes() == want[0].tobytes()
    return {"records": len(fr), "summary": got[3], "calls": reps,
            "kernel_ms_median": {k: round(statistics.median(v), 5) for k, v in sorted(kernels.items())},
            "kernel_ms_min": {k: round(min(v), 5) for k, v in sorted(kernels.items())},
            "call_wall_ms_median": round(statistics.median(wall), 4), "call_wall_ms_min": round(min(wall), 4),
            "host_wall_ms_median": round(statistics.median(host), 4), "host_wall_ms_min": round(min(host), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    pdt = importlib.import_module("project-desert-tortoise_amd")
    res = {"build": pdt.build_tag(), "tile": pdt.tip_subcom_tile()}
    sets = {"pass_frames": records(pdt, pdt.synth_params(0, 250000, 1000.0, 1234), 600, 7800),
            "kind4_hour": records(pdt, pdt.synth_params(4, 50000, 1000.0, 7), 0, 36000)}
    tables = {"sem": pdt.SUBCOM_SEM, "hk": pdt.SUBCOM_HK, "wide_256": wide_table(pdt)}
    with pdt.Demodulator(pdt.MODE_POES, 250000, profile=True) as d:
        for sname, fr in sets.items():
            for tname, table in tables.items():
                res[f"{sname}.{tname}"] = measure(pdt, d, fr, table, a.reps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
