#!/usr/bin/env python3
"""Rate of the fully observable encoding (k_full_obs; BatchedBabyAIEnv(full_obs=True)): per workload, HIP-event medians after warm-up of
  - observe_full() of every env (bbai_observe_full: the kernel alone),
  - step() with full_obs=True (bbai_step_full: k_step + k_full_obs as one call) and with full_obs=False (bbai_step) on twin batches,
    alternated block by block,
and the achieved rate on the algorithmic bytes of a frame: 3 W H stored + W H appearance bytes + the 16-byte Hot read per env (BossLevel:
1 952 B).  One JSON line per workload, to stdout and to --out.

    python tools/full_obs_bench.py [--reps 30] [--only gotolocal,pickuploc,boss] [--out profiles/full_obs/full_obs_bench.jsonl]

Under `rocprofv3 --kernel-trace --stats` (or a `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` pass) the same command gives the kernel's own time /
traffic.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "gotolocal": ("GoToLocal", 65536),
    "pickuploc": ("PickupLoc", 262144),
    "boss": ("BossLevel", 1048576),
}
PEAK_TBS = 8.0


def timed(torch, fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    out = open(args.out, "a") if args.out else None
    for name in args.only.split(","):
        level, n = WORKLOADS[name]
        full = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device="cuda:0", seeds=1, full_obs=True)
        plain = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device="cuda:0", seeds=1)
        full.reset()
        plain.reset()
        c = full.cfg
        rng = np.random.RandomState(0)
        acts = [torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device="cuda:0") for _ in range(16)]
        for t in range(args.warmup):
            full.step(acts[t % 16])
            plain.step(acts[t % 16])
            full.observe_full()
        torch.cuda.synchronize()
        obs_ms = timed(torch, lambda: full.observe_full(), args.reps)
        step_full, step_plain = [], []
        for r in range(args.reps):            # alternated: the twin batches see the same box state
            step_full += timed(torch, lambda: full.step(acts[r % 16]), 1)
            step_plain += timed(torch, lambda: plain.step(acts[r % 16]), 1)
        frame = 3 * c.W * c.H
        algo = n * (frame + c.W * c.H + 16)
        med = float(np.median(obs_ms))
        line = {"workload": name, "level": level, "envs": n, "W": c.W, "H": c.H, "frame_bytes": frame, "algorithmic_bytes_per_env": frame + c.W * c.H + 16,
                "algorithmic_bytes": algo, "observe_full_ms_median": round(med, 4), "observe_full_ms_min": round(min(obs_ms), 4),
                "TB_per_s_algorithmic": round(algo / med / 1e9, 3), "frac_of_8TBs": round(algo / med / 1e9 / PEAK_TBS, 3),
                "step_full_ms_median": round(float(np.median(step_full)), 4), "step_plain_ms_median": round(float(np.median(step_plain)), 4),
                "step_full_minus_plain_ms": round(float(np.median(step_full)) - float(np.median(step_plain)), 4), "reps": args.reps}
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
        full.close()
        plain.close()
        del full, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
