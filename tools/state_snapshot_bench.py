#!/usr/bin/env python3
"""Cost of device snapshots (k_state_save / k_state_load, include/bbai.h bbai_save_state / bbai_load_state): per workload, HIP-event time per
call of save_state / load_state for every env and for 4 096 and 64 scattered envs, the bytes each call has to move, the resulting rate -- and,
in the same process and alternated with them, what the host path costs for the same envs (export_state + import_state of the contiguous range
that covers them: wall clock, it synchronises) and, for the all-env case, a Tensor.copy_ of the same bytes.  Every figure is the mean over at
least --min-seconds of timed calls on warm shapes; `runs` holds the repeated figures, median first.  The last lines compare a 64-env load in a
4 096-env batch and in the large one: the call's grid follows the list, so the two must agree within their own spread.  One JSON line per figure.

    python tools/state_snapshot_bench.py [--only boss,local] [--out profiles/state_snapshot/state_snapshot_bench.jsonl]
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
    "boss": ("BossLevel", 1048576),
    "local": ("GoToLocal", 65536),
}
LISTS = (4096, 64)


def event_ms(torch, call, min_seconds, repeats=3):
    """ms per call: `repeats` timed batches of back-to-back calls, each at least min_seconds long; (median, all)."""
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
    ap.add_argument("--pairs", type=int, default=2, help="alternations of the device calls with the host path")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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

    def row_bytes(env):
        return env.cfg.rec_bytes + 16 + 8 + 1

    def load64(env, name, n):
        ids = torch.as_tensor(np.sort(np.random.RandomState(64).choice(n, 64, replace=False)), device=dev)
        snap = env.save_state(ids)
        med, runs, reps = event_ms(torch, lambda: env.load_state(snap, ids=ids), args.min_seconds, repeats=5)
        emit({"workload": name, "figure": "load_64_scattered", "envs": n, "listed": 64, "ms": med, "runs_ms": runs, "calls_per_run": reps,
              "bytes_moved": 64 * (2 * row_bytes(env) + 148)})
        return med, runs

    for name in args.only.split(","):
        level, n = WORKLOADS[name]
        env = make(level, n)
        rb = row_bytes(env)
        # a load reads the row, writes it, and writes the 147-byte observation + direction (+ what the handle derives: not counted)
        for k in (n,) + LISTS:
            host_ids = None if k == n else np.sort(np.random.RandomState(k).choice(n, k, replace=False))
            ids = None if host_ids is None else torch.as_tensor(host_ids, device=dev)
            first, count = (0, n) if host_ids is None else (int(host_ids[0]), int(host_ids[-1] - host_ids[0] + 1))
            what = "all" if k == n else "%d_scattered" % k
            snap = env.save_state(ids)

            def host_path():
                rec, hot, stale = env.export_state(first, count)
                env.import_state(rec, hot, stale, first)

            for pair in range(args.pairs):
                s_med, s_runs, s_reps = event_ms(torch, lambda: env.save_state(ids), args.min_seconds)
                l_med, l_runs, l_reps = event_ms(torch, lambda: env.load_state(snap, ids=ids), args.min_seconds)
                h_ms, h_calls = wall_ms(torch, host_path, args.min_seconds)
                emit({"workload": name, "figure": "save_" + what, "pair": pair, "envs": n, "listed": k, "ms": s_med, "runs_ms": s_runs, "calls_per_run": s_reps,
                      "bytes_moved": 2 * k * rb, "GB_per_s": 2 * k * rb / s_med / 1e6})
                emit({"workload": name, "figure": "load_" + what, "pair": pair, "envs": n, "listed": k, "ms": l_med, "runs_ms": l_runs, "calls_per_run": l_reps,
                      "bytes_moved": k * (2 * rb + 148), "GB_per_s": k * (2 * rb + 148) / l_med / 1e6})
                emit({"workload": name, "figure": "host_export_import_" + what, "pair": pair, "envs": n, "listed": k, "covering_range": count, "ms_wall": h_ms,
                      "calls": h_calls, "bytes_through_host": 2 * count * (rb - 1), "speedup_save_plus_load": h_ms / (s_med + l_med)})
            if k == n:
                dst = [torch.empty_like(t) for t in (snap.rec, snap.hot, snap.stale, snap.lsm)]

                def copy():
                    for d, s in zip(dst, (snap.rec, snap.hot, snap.stale, snap.lsm)):
                        d.copy_(s)
                c_med, c_runs, c_reps = event_ms(torch, copy, args.min_seconds)
                emit({"workload": name, "figure": "tensor_copy_all", "envs": n, "ms": c_med, "runs_ms": c_runs, "calls_per_run": c_reps, "bytes_moved": 2 * k * rb,
                      "GB_per_s": 2 * k * rb / c_med / 1e6})
                del dst
            del snap
        big, big_runs = load64(env, name, n)
        env.close()
        del env
        torch.cuda.empty_cache()
        small_env = make(level, 4096)
        small, small_runs = load64(small_env, name, 4096)
        small_env.close()
        lo, hi = min(big_runs + small_runs), max(big_runs + small_runs)
        emit({"workload": name, "figure": "load_64_by_batch_size", "ms_at_4096": small, "ms_at_%d" % n: big, "runs_ms_at_4096": small_runs, "runs_ms_at_%d" % n: big_runs,
              "spread_of_runs_ms": max(max(big_runs) - min(big_runs), max(small_runs) - min(small_runs)), "difference_ms": abs(big - small),
              "all_runs_ms_min_max": [lo, hi]})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
