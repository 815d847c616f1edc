"""The flywheel synchroniser's kernels on the GPU, from pdt_kernel_times of a profiled context, on two inputs:

(a) a bit string of --bits bits (30 M: what an hour-long POES capture leaves) through pdt_stage_tip_sync -- the bits of a weak 30 s
    synthetic capture, demodulated here, repeated end to end
(b) --batch contexts (16) of 12 s captures demodulated by one pdt_demod_batch_device call, one pdt_tip_sync_batch call

--reps calls of each; the first carries the kernels' first-use cost and is reported with the others, in order.  One JSON to --out.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("k_tip_cand", "k_tip_heads", "k_tip_pick", "k_tip_scan", "k_tip_pack")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bits", type=int, default=30_000_000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch
    pdt = importlib.import_module("project-desert-tortoise_amd")
    import test_tip_sync as cpu
    result = {"build": pdt.build_tag(), "kernels": NAMES}

    def ms(times):
        return [round(times[name][1], 4) for name in NAMES]

    with pdt.Demodulator(pdt.MODE_POES, 50000, profile=True) as d:
        d.demod(cpu.weak_capture(pdt)[1])
        one = d.stage(pdt.ST_BITS)
        bits = np.tile(one, args.bits // len(one) + 1)[:args.bits]
        runs, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fr, found = d.stage_tip_sync(bits, with_count=True)
            wall.append(round(1e3 * (time.perf_counter() - t0), 2))
            runs.append(ms(d.kernel_times()))
        result["long_string"] = {"bits": len(bits), "frames": found, "ms_per_kernel": runs, "ms_call_with_upload": wall}

    caps = [cpu.weak_capture(pdt, 6 if k % 2 else 9, 100 + k, 12.0)[1] for k in range(args.batch)]
    dev = [torch.from_numpy(iq.reshape(-1).copy()).to("cuda:0") for iq in caps]
    torch.cuda.synchronize()
    ds = [pdt.Demodulator(pdt.MODE_POES, 50000, profile=(i == 0)) for i in range(args.batch)]
    try:
        pdt.demod_batch(ds, [t.data_ptr() for t in dev], [len(iq) for iq in caps])
        runs, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = pdt.tip_sync_batch(ds)
            wall.append(round(1e3 * (time.perf_counter() - t0), 2))
            runs.append(ms(ds[0].kernel_times()))
        result["batch"] = {"contexts": args.batch, "bits": [int(d.stage_len(pdt.ST_BITS)) for d in ds], "frames": [len(g) for g in got],
                           "rule0_frames": [int(d.frames_array()["complete"].sum()) for d in ds], "ms_per_kernel": runs, "ms_call": wall}
    finally:
        for d in ds:
            d.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
