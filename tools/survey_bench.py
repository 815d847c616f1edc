"""The carrier survey of wideband captures: a 15-minute 2.4 Msps unsigned 8-bit capture resident in HBM (the capture of
tools/channel_bench.py), surveyed at --nfft; wall time of the whole call (kernels, read-back of the spectrum, the host's search),
median of --reps, and the carriers found.

Run it under `rocprofv3 --kernel-trace --stats -d DIR -o survey -- python tools/survey_bench.py --nfft N` for the kernels' own time
(k_spectra and k_survey_sum in DIR/.../survey_kernel_stats.csv); `--stats FILE --nfft N` then turns that file's rows into time per call
and bytes read over time (2 B per input sample, read once), as a share of the 6.3 TB/s measured for a float4 copy.
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


def kernel_share(path: str, n: int, nfft: int) -> dict:
    with open(path) as f:
        rows = list(csv.DictReader(f))
    out = {"nfft": nfft}
    for key, name in (("survey", "k_spectra"), ("sum", "k_survey_sum")):
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        out[f"{key}_kernel_ms"] = round(sum(float(r["TotalDurationNs"]) for r in sel) / max(calls, 1) / 1e6, 3)
        out[f"{key}_calls"] = calls
    tb_s = 2.0 * (n // nfft * nfft) / (out["survey_kernel_ms"] * 1e-3) / 1e12
    out.update({"read_TB_s": round(tb_s, 4), "of_6.3": round(tb_s / 6.3, 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=900.0)
    ap.add_argument("--rate", type=int, default=2400000)
    ap.add_argument("--decim", type=int, default=16)
    ap.add_argument("--nfft", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run: print the kernels' time and read rate")
    a = ap.parse_args()
    n = int(a.seconds * a.rate)
    if a.stats:
        print(json.dumps(kernel_share(a.stats, n, a.nfft)))
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
    out = {"samples": n, "rate": a.rate, "nfft": a.nfft}
    with pdt.Demodulator(pdt.MODE_POES, a.rate // a.decim) as d:
        d.set_channel(a.decim, 0.0)
        found = d.survey_device(dev.data_ptr(), n, pdt.FMT_WB_CU8, nfft=a.nfft)        # (buffers allocated once)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            found = d.survey_device(dev.data_ptr(), n, pdt.FMT_WB_CU8, nfft=a.nfft)
            ts.append((time.perf_counter() - t0) * 1e3)
    out["call_ms"] = round(float(np.median(ts)), 2)
    out["carriers"] = [[round(c.offset_hz, 1), round(float(c.peak_db), 1)] for c in found]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
