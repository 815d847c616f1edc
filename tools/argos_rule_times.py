"""The message kernels of both rules on the same GPU in alternating calls: k_argos_msgs and k_argos_finish (rule 0) beside
k_argos_heads and k_argos_pick (rule 1), from pdt_kernel_times of a profiled context, on the two inputs of profiles/r17:

(a) the windows of a two-platform kind-2 capture (48 s at 1.024 Msps, decimation 32: 64 windows), one pdt_argos_messages_batch call
(b) the 5-minute ARGOS capture of `bench.py --config argos` (9.6 M samples at 32 ksps), one pdt_argos_messages call

--reps calls of each rule, rule 0 and rule 1 in turn; the first call of each carries the kernels' first-use cost and is reported with
the others, in order.  One JSON to --out.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = {0: ("k_argos_msgs", "k_argos_finish"), 1: ("k_argos_heads", "k_argos_pick")}


def alternate(call, times, reps: int):
    """reps x (rule 0, rule 1): per rule the list of (search ms, selection ms) and the number of messages of the last call"""
    runs, found = {0: [], 1: []}, {}
    for _ in range(reps):
        for rule in (0, 1):
            found[rule] = call(rule)
            t = times()
            runs[rule].append([round(t[name][1], 4) for name in NAMES[rule]])
    return runs, found


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=48.0)
    ap.add_argument("--seeds", type=int, nargs=2, default=(206, 210))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    pdt = importlib.import_module("project-desert-tortoise_amd")
    import argos_best_cases as bc
    result = {"build": pdt.build_tag(), "kernels": NAMES}

    x, params = bc.kind2_pair(pdt, tuple(args.seeds), args.seconds)
    with pdt.Demodulator(pdt.MODE_ARGOS, bc.FS) as holder:
        holder.set_channel(bc.D, 0.0)
        windows = pdt.burst_windows(holder.bursts(x), bc.IN_RATE, len(x))
        ds = [pdt.Demodulator(pdt.MODE_ARGOS, bc.FS, profile=(i == 0)).set_channel(bc.D, 0.0) for i in range(len(windows))]
        try:
            pdt.demod_windows(ds, x, 0, 0, windows)
            last = {}

            def call(rule):
                last[rule] = pdt.argos_messages_batch(ds, rule=rule)
                return sum(len(m) for m in last[rule])

            runs, found = alternate(call, ds[0].kernel_times, args.reps)
            result["windows"] = {"count": len(windows), "seeds": list(args.seeds), "seconds": args.seconds,
                                 "bits": [int(d.stage_len(pdt.ST_BITS)) for d in ds[:8]], "messages": found,
                                 "right_windows": {rule: bc.tally(pdt, params, windows, last[rule])[0] for rule in (0, 1)},
                                 "ms_search_selection": runs}
        finally:
            for d in ds:
                d.close()
    del x

    y = pdt.synth_capture(1, 32000, 300.0)
    with pdt.Demodulator(pdt.MODE_ARGOS, 32000, profile=True) as d:
        d.demod(y)
        runs, found = alternate(lambda rule: len(d.argos_messages(rule=rule, cap=8192)), d.kernel_times, args.reps)
        result["argos_5min"] = {"samples": len(y), "bits": int(d.stage_len(pdt.ST_BITS)), "frames": len(d.frames_array()), "messages": found,
                                "ms_search_selection": runs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
