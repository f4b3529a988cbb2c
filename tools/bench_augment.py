#!/usr/bin/env python
"""hyperparameter_search's sampling call on the device: DeviceMeshAugmentation.sampling(40000, q, pool=10), the
sampling_main(10, 40000, q) of general/EBRD.py's data_sampling, at q = 0.7 and q = 0.8.

Per threshold: WARMUP calls, then ROUNDS timed calls, each a different seed (a call's work depends on its streams), a host clock
around a device synchronise; medians and interquartile ranges of the wall time and of the device's own tallies (proposals drawn,
candidates scored, rounds).  There is no parent-commit time and no reference on the GPU machine, so no ratio is formed here;
`reference_context` repeats what tools/gen_augment_golden.py measured for the reference's sampling(440, 0.7) on one CPU core
of another machine, as context only.  Per-kernel times come from a separate rocprofv3 --kernel-trace --stats run of
`--rounds 1 --warmup 1`.

    python tools/bench_augment.py [--out profiles/augment_bench.json] [--n 40000] [--pool 10] [--rounds 9] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from reinforcementlearning4meshgeneration_amd import DeviceMeshAugmentation  # noqa: E402
from reinforcementlearning4meshgeneration_amd.augmentation import row_count  # noqa: E402

THRESHOLDS = (0.7, 0.8)


def quartiles(v, digits=3):
    q = statistics.quantiles(v, n=4)
    return dict(median=round(statistics.median(v), digits), iqr=round(q[2] - q[0], digits), min=round(min(v), digits), max=round(max(v), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--pool", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--round-size", type=int, default=8192)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augment needs a ROCm GPU: there is no CPU fallback")
    from source_state import state
    aug = DeviceMeshAugmentation()
    R = row_count(args.n, args.pool)
    per_threshold = {}
    for thr in THRESHOLDS:
        ms, tallies = [], {k: [] for k in ("proposals", "candidates", "rounds")}
        for r in range(args.warmup + args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, y = aug.sampling(args.n, thr, seed=1000 + r, pool=args.pool, round_size=args.round_size)
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            assert len(x) == R == aug.last_stats["rows"]
            if r >= args.warmup:
                ms.append(dt)
                for k in tallies:
                    tallies[k].append(aug.last_stats[k])
        per_threshold[str(thr)] = dict(wall_ms=quartiles(ms) if len(ms) > 1 else dict(median=round(ms[0], 3)), rows=R,
                                       **{k: (quartiles(v, 0) if len(v) > 1 else dict(median=v[0])) for k, v in tallies.items()})
    counts = json.load(open(os.path.join(ROOT, "tests", "golden", "augment_counts.json")))["n"]["440"]
    summary = dict(summary="bench_augment", device=torch.cuda.get_device_name(0), n=args.n, pool=args.pool, round_size=args.round_size,
                   rounds=args.rounds, warmup=args.warmup, **state(), sampling=per_threshold,
                   reference_context=dict(call="sampling(440, 0.7)", rows=counts["rows"], seconds_one_cpu_core=counts["reference_seconds_one_core"],
                                          note="the reference on one CPU core of a different machine: context, not a comparison"))
    with open(args.out, "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    print(json.dumps(summary), flush=True)
    aug.close()


if __name__ == "__main__":
    main()
