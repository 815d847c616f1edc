"""The feed-forward kernels on one round of per-burst windows: k_ff_mix, k_ff_search and k_ff_pick from pdt_kernel_times of a
profiled context and the wall time of the whole pdt_ff_messages_batch call, beside the wall time of what gives the loop's messages for
the same round -- pdt_demod_windows_held (the down-converter and the chain) plus pdt_argos_messages_batch -- on the windows of
profiles/r18/argos_times.json: a two-platform kind-2 capture, 48 s at 1.024 Msps, decimation 32.

--reps calls of each, in turn; the first call carries the kernels' first-use cost and the buffers' allocation and is reported with the
others, in order.  The feed-forward call needs the channel streams that pdt_demod_windows_held leaves: a round that skips the chain does
not exist, so its time is not a replacement's but an addition's.  One JSON to --out.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("k_ff_mix", "k_ff_search", "k_ff_pick")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=48.0)
    ap.add_argument("--seeds", type=int, nargs=2, default=(206, 210))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pdt = importlib.import_module("project-desert-tortoise_amd")
    import argos_best_cases as bc
    result = {"build": pdt.build_tag(), "kernels": NAMES, "seeds": list(args.seeds), "seconds": args.seconds}

    x, params = bc.kind2_pair(pdt, tuple(args.seeds), args.seconds)
    with pdt.Demodulator(pdt.MODE_ARGOS, bc.FS) as holder:
        holder.set_channel(bc.D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x), bc.IN_RATE, len(x))
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, bc.FS, profile=(i == 0)).set_channel(bc.D, 0.0) for i in range(len(windows))]
        try:
            runs = {"ff_kernels_ms": [], "ff_messages_batch_wall_ms": [], "demod_windows_held_wall_ms": [], "argos_messages_batch_wall_ms": []}
            for _ in range(args.reps):
                t0 = time.perf_counter()
                holder.demod_windows_held(ds, windows)
                t1 = time.perf_counter()
                loop = pdt.argos_messages_batch(ds)
                t2 = time.perf_counter()
                ff = pdt.ff_messages_batch(ds)
                t3 = time.perf_counter()
                times = ds[0].kernel_times()
                runs["ff_kernels_ms"].append([round(times[name][1], 4) for name in NAMES])
                runs["demod_windows_held_wall_ms"].append(round((t1 - t0) * 1e3, 3))
                runs["argos_messages_batch_wall_ms"].append(round((t2 - t1) * 1e3, 3))
                runs["ff_messages_batch_wall_ms"].append(round((t3 - t2) * 1e3, 3))
            result["windows"] = len(windows)
            result["samples"] = [int(d.stage_len(pdt.ST_CHANNEL)) for d in ds[:8]]
            result["ff_bits"] = [int(len(d.ff_read().bits)) for d in ds[:8]]
            result.update(runs)
            result["right_wrong"] = {}
            for name, msgs in (("loop_first", loop), ("loop_best", pdt.argos_messages_batch(ds, rule=1)), ("ff_first", ff),
                               ("ff_best", pdt.ff_messages_batch(ds, rule=1))):
                right, wrong, lost = bc.tally(pdt, params, windows, msgs)
                result["right_wrong"][name] = {"right": right, "wrong": wrong, "not_right_at_frame": lost}
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
