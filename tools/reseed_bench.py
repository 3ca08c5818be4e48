#!/usr/bin/env python3
"""Cost of bbai_reseed (k_reseed_seed, the generators over the reseed's work list, k_reseed_consume; include/bbai.h): per workload, HIP-event time
per `reseed` call for 64 and 4 096 scattered envs and for every env, at the workload's default look-ahead period and at BBAI_LOOKAHEAD=4 -- and,
in the same process and alternated with them, the only way to give envs new seeds without it: `seed()` + `reset()` of the whole batch (wall
clock: bbai_seed synchronises).  A reseed generates the listed envs' WHOLE rings (ring depth D levels each, one env's in sequence), so its latency
is bounded below by D levels of one lane group / lane however few envs are listed: the 64-env figure is that latency.  Every figure is the mean
over at least --min-seconds of back-to-back calls on warm shapes; `runs_ms` holds the repeated figures, `ms` their median.  One JSON line per
figure.  --levels K[,K ...]: SHORT reseeds instead (reseed(ids, seeds, levels=K): K levels per listed env and a parking slot behind them) -- the
64- and 4 096-env lists at depth 0 (the whole ring) and at every K, alternated on the same handle; the whole-batch figures are left out.

    python tools/reseed_bench.py [--only local,boss,goto] [--levels 1] [--out profiles/reseed/reseed_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: level, envs in the batch
WORKLOADS = {
    "local": ("GoToLocal", 65536),
    "boss": ("BossLevel", 1048576),
    "goto": ("GoTo", 131072),
}
LISTS = (64, 4096)


def event_ms(torch, call, min_seconds, repeats=3):
    """ms per call: `repeats` timed batches of back-to-back calls, each at least min_seconds long; (median, all, calls per batch)."""
    call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); call(); b.record(); b.synchronize()
    reps = max(1, int(min_seconds * 1e3 / max(a.elapsed_time(b), 1e-3)) + 1)
    runs = []
    for _ in range(repeats):
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) / reps)
    return sorted(runs)[len(runs) // 2], runs, reps


def wall_ms(torch, call, min_seconds):
    torch.cuda.synchronize()
    t0, k = time.perf_counter(), 0
    while True:
        call()
        k += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt * 1e3 / k, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--pairs", type=int, default=2, help="alternations of the reseed calls with seed() + reset()")
    ap.add_argument("--levels", default=None, help="comma-separated reseed depths to alternate with depth 0 (the whole ring)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    depths = [int(v) for v in args.levels.split(",")] if args.levels else None
    import numpy as np
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    dev = "cuda:0"
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def make(level, n):
        env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=dev, seeds=1)
        env.reset()
        rng = np.random.RandomState(0)
        for _ in range(8):
            env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=dev))
        return env

    for name in args.only.split(","):
        level, n = WORKLOADS[name]
        for lookahead in (None, 4):
            if lookahead is None:
                os.environ.pop("BBAI_LOOKAHEAD", None)
            else:
                os.environ["BBAI_LOOKAHEAD"] = str(lookahead)
            env = make(level, n)
            shape = {"workload": name, "level": level, "envs": n, "lookahead_period": env.get_option("lookahead_period"),
                     "inplace": env.get_option("inplace"), "pregen_lane": env.get_option("pregen_lane")}
            shape["ring_depth"] = 2 * shape["lookahead_period"] + shape["inplace"]
            all_seeds = np.arange(n, dtype=np.uint64) + np.uint64(10 ** 6)

            def whole_batch():
                env.seed(all_seeds)
                env.reset()

            full = shape["ring_depth"] - shape["inplace"]
            for pair in range(args.pairs if depths else 0):
                for k in LISTS:
                    ids = torch.as_tensor(np.sort(np.random.RandomState(k).choice(n, k, replace=False)), device=dev)
                    seeds = torch.as_tensor((np.arange(k, dtype=np.int64) * 3 + 5 * 10 ** 6 + pair), device=dev)
                    for depth in [0] + depths:
                        med, runs, reps = event_ms(torch, lambda: env.reseed(ids, seeds, levels=depth), args.min_seconds)
                        gen = depth if 0 < depth < full else full
                        emit(dict(shape, figure="reseed_%d_scattered" % k, reseed_levels=depth, pair=pair, listed=k, ms=med, runs_ms=runs, calls_per_run=reps,
                                  levels_generated=k * gen, us_per_level_of_one_env=med * 1e3 / gen))
            for pair in range(0 if depths else args.pairs):
                for k in LISTS + ((n,) if lookahead is None else ()):
                    ids = None if k == n else torch.as_tensor(np.sort(np.random.RandomState(k).choice(n, k, replace=False)), device=dev)
                    seeds = torch.as_tensor((np.arange(k, dtype=np.int64) * 3 + 5 * 10 ** 6 + pair), device=dev)
                    med, runs, reps = event_ms(torch, lambda: env.reseed(ids, seeds), args.min_seconds)
                    emit(dict(shape, figure="reseed_all" if k == n else "reseed_%d_scattered" % k, pair=pair, listed=k, ms=med, runs_ms=runs, calls_per_run=reps,
                              levels_generated=k * (shape["ring_depth"] - shape["inplace"]), us_per_level_of_one_env=med * 1e3 / (shape["ring_depth"] - shape["inplace"])))
                if lookahead is None and not depths:
                    w_ms, calls = wall_ms(torch, whole_batch, args.min_seconds)
                    emit(dict(shape, figure="seed_plus_reset_whole_batch", pair=pair, listed=n, ms_wall=w_ms, calls=calls))
            assert env.get_option("gate_timeouts") == 0
            env.close()
            del env
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
