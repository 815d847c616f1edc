"""The down-converter of wideband captures: a 15-minute 2.4 Msps unsigned 8-bit capture resident in HBM, decimation 16,
K channels of it (pdt_demod_channels_device), wall time of the whole call, median of --reps, and that time per channel.

Run it under `rocprofv3 --kernel-trace --stats -d DIR -o ddc -- python tools/channel_bench.py --channels K` for the conversion
kernel's own time (k_ddc in DIR/.../ddc_kernel_stats.csv); `--stats FILE --channels K` then turns that file's k_ddc row into the
kernel time of one demod_channels call -- K launches, one per channel -- and into bytes read over that time (2 B per input sample
and channel), as a share of the 6.3 TB/s measured for a float4 copy.  The capture is 30 s of four synthetic POES carriers, repeated
on the device.
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


def kernel_share(path: str, n: int, k: int) -> dict:
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_ddc" in r["Name"]]
    ns = sum(float(r["TotalDurationNs"]) for r in rows)
    launches = sum(int(r["Calls"]) for r in rows)
    calls = launches // k                                  # one launch per channel of a demod_channels call
    per_call_ms = ns / calls / 1e6
    tb_s = 2.0 * n * k / (per_call_ms * 1e-3) / 1e12
    return {"channels": k, "kernel_ms": round(per_call_ms, 3), "calls": calls, "launches": launches, "read_TB_s": round(tb_s, 4),
            "of_6.3": round(tb_s / 6.3, 4), "out_GB": round(8.0 * k * n / 16 / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=900.0)
    ap.add_argument("--rate", type=int, default=2400000)
    ap.add_argument("--decim", type=int, default=16)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run: print the kernel's time and read rate")
    a = ap.parse_args()
    n = int(a.seconds * a.rate)
    if a.stats:
        print(json.dumps(kernel_share(a.stats, n, a.channels)))
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
    fs = a.rate // a.decim
    ds = [pdt.Demodulator(pdt.MODE_POES, fs).keep_pll(False).set_channel(a.decim, off) for off in OFFSETS[: a.channels]]
    out = {"samples": n, "rate": a.rate, "decim": a.decim, "channels": a.channels}
    pdt.demod_channels(ds, dev.data_ptr(), n, pdt.FMT_WB_CU8)                 # (buffers of this size allocated once)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        pdt.demod_channels(ds, dev.data_ptr(), n, pdt.FMT_WB_CU8)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["call_ms"] = round(float(np.median(ts)), 2)
    out["call_ms_per_channel"] = round(float(np.median(ts)) / a.channels, 2)
    out["frames"] = [int(d.stats().frames) for d in ds]
    for d in ds:
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
