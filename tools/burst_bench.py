"""The burst search of wideband captures: the 15-minute 2.4 Msps unsigned 8-bit capture of tools/survey_bench.py resident
in HBM, searched at --nfft and --rows-per; wall time of the whole call (the survey for the floor, the slabs' kernels, read-back of the
peaks, the host's linking), median of --reps, and the number of bursts found.

Run it under `rocprofv3 --kernel-trace --stats -d DIR -o bursts -- python tools/burst_bench.py --nfft N --rows-per R` for the kernels'
own time; `--stats FILE` then turns that file's rows into the total time and the launches of k_spectra, k_row_peaks and k_survey_sum.
A burst search of S slabs launches k_spectra 1 + S times -- once over the stretch in runs of 64 segments for the floor, once per slab
for the rows: one kernel, one name -- and k_row_peaks S times.
"""
import argparse
import csv
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OFFSETS = (600000.0, -400000.0, 250000.0, -850000.0)


def kernel_times(path: str, calls: int) -> dict:
    """ms per call of the bench's searches (calls = reps + 1: the first call allocates) for each kernel of the trace"""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for key in ("k_spectra", "k_row_peaks", "k_survey_sum"):
                if key in r["Name"]:
                    out[key + "_ms"] = round(out.get(key + "_ms", 0.0) + float(r["TotalDurationNs"]) / 1e6, 3)
                    out[key + "_launches"] = out.get(key + "_launches", 0) + int(r["Calls"])
                    break
    out["calls"] = calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=900.0)
    ap.add_argument("--rate", type=int, default=2400000)
    ap.add_argument("--decim", type=int, default=16)
    ap.add_argument("--nfft", type=int, default=4096)
    ap.add_argument("--rows-per", type=int, default=8)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run: print the kernels' total time and launches")
    a = ap.parse_args()
    n = int(a.seconds * a.rate)
    if a.stats:
        print(json.dumps(kernel_times(a.stats, a.reps + 1)))
        return
    import torch
    pdt = importlib.import_module("project-desert-tortoise_amd")
    base_n = min(n, 30 * a.rate)
    total = np.zeros((base_n, 2), dtype=np.int32)
    for i, off in enumerate(OFFSETS):
        p = pdt.synth_params(0, a.rate, off + 1000.0, 11 + i)
        p.amplitude //= 4
        p.noise_gain //= 4
        iq = np.zeros((base_n, 2), dtype="<i2")
        pdt.synth_lib().pdt_synth_fill(C.byref(p), 0, base_n, iq.ctypes.data)
        total += iq
    u8 = np.clip(np.floor(total / 256.0) + 128, 0, 255).astype(np.uint8)
    piece = torch.from_numpy(u8.reshape(-1)).cuda()
    dev = piece.repeat((n + base_n - 1) // base_n)[: 2 * n].contiguous()
    del piece, total, u8
    torch.cuda.synchronize()
    out = {"samples": n, "rate": a.rate, "nfft": a.nfft, "rows_per": a.rows_per}
    with pdt.Demodulator(pdt.MODE_POES, a.rate // a.decim) as d:
        d.set_channel(a.decim, 0.0)
        cfg = dict(nfft=a.nfft, rows_per=a.rows_per, cap=1 << 16)
        found = d.bursts_device(dev.data_ptr(), n, pdt.FMT_WB_CU8, **cfg)                # (buffers allocated once)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            found = d.bursts_device(dev.data_ptr(), n, pdt.FMT_WB_CU8, **cfg)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["call_ms"] = round(float(np.median(ts)), 2)
        out["bursts"] = len(found)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
