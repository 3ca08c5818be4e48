#!/usr/bin/env python3
"""Rate of the partial-view render at tile sizes 16 and 32 (k_view_pixels, include/bbai.h bbai_render_view): per workload, the median
over timed calls of HIP-event time, the frame bytes stored per call and the resulting store rate -- and, in the same process, a plain
Tensor.fill_ of the same byte count and k_render_grid at the same tile size over about as many bytes.  One JSON line per workload.

    python tools/view_render_bench.py [--reps 20] [--only boss16,boss32]

Under `rocprofv3 --kernel-trace --stats` (or, in a run of its own, a `--pmc WRITE_SIZE` pass) the same command gives the kernel's own
time / stored bytes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: level, envs in the batch (all rendered), tile size
WORKLOADS = {
    "boss16": ("BossLevel", 65536, 16),
    "boss32": ("BossLevel", 8192, 32),
}


def timed(torch, np, reps, call):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--no-grid", action="store_true", help="skip the k_render_grid comparison")
    args = ap.parse_args()
    import numpy as np
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    for name in args.only.split(","):
        level, n, ts = WORKLOADS[name]
        env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device="cuda:0", seeds=1)
        env.reset()
        rng = np.random.RandomState(0)
        for _ in range(8):
            env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device="cuda:0"))
        out = env.render_view(None, tile_size=ts)
        nbytes = out.numel()
        med, lo = timed(torch, np, args.reps, lambda: env.render_view(None, tile_size=ts, out=out))
        fill_med, _ = timed(torch, np, args.reps, lambda: out.fill_(7))
        rec = {"workload": name, "level": level, "envs": n, "tile_size": ts, "frame_bytes": nbytes // n, "bytes_per_call": nbytes,
               "ms_median": round(med, 4), "ms_min": round(lo, 4), "TB_per_s": round(nbytes / med / 1e9, 3),
               "fill_ms_median": round(fill_med, 4), "fill_TB_per_s": round(nbytes / fill_med / 1e9, 3), "fraction_of_fill": round(fill_med / med, 3)}
        if not args.no_grid:
            c = env.cfg
            gf = c.H * ts * c.W * ts * 3
            k = max(1, min(n, nbytes // gf))
            ids = torch.as_tensor(rng.choice(n, k, replace=False).astype(np.int64), device="cuda:0")
            gout = out.reshape(-1)[:k * gf].reshape(k, c.H * ts, c.W * ts, 3)          # (the same memory: no second buffer of that size)
            gmed, _ = timed(torch, np, args.reps, lambda: env.render_grid(ids, tile_size=ts, highlight=True, out=gout))
            rec.update({"grid_frames": k, "grid_bytes_per_call": k * gf, "grid_ms_median": round(gmed, 4), "grid_TB_per_s": round(k * gf / gmed / 1e9, 3)})
        print(json.dumps(rec), flush=True)
        del out
        env.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
