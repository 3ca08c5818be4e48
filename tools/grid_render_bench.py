#!/usr/bin/env python3
"""Rate of the full-grid picture (k_render_grid, BatchedBabyAIEnv.render_grid): per workload, the median over timed calls of HIP-event
time, the frame bytes stored per call and the resulting store rate.  One JSON line per workload.

    python tools/grid_render_bench.py [--reps 20] [--only gotolocal,boss8,boss32]

Under `rocprofv3 --kernel-trace --stats` (or a `--pmc WRITE_SIZE` pass) the same command gives the kernel's own time / stored bytes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: level, envs in the batch, envs rendered (None = all), tile size
WORKLOADS = {
    "gotolocal": ("GoToLocal", 65536, None, 8),
    "boss8": ("BossLevel", 131072, None, 8),
    "boss32": ("BossLevel", 131072, 64, 32),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--bpc", type=int, default=0, help="option grid_render_bpc (0 = the default)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    for name in args.only.split(","):
        level, n, k, ts = WORKLOADS[name]
        env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device="cuda:0", seeds=1)
        env.reset()
        if args.bpc:
            env.set_option("grid_render_bpc", args.bpc)
        rng = np.random.RandomState(0)
        for _ in range(8):
            env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device="cuda:0"))
        ids = None if k is None else torch.as_tensor(rng.choice(n, k, replace=False).astype(np.int64), device="cuda:0")
        out = env.render_grid(ids, tile_size=ts, highlight=True)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            env.render_grid(ids, tile_size=ts, highlight=True, out=out)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        nbytes = out.numel()
        print(json.dumps({"workload": name, "level": level, "envs": n, "rendered": int(out.shape[0]), "tile_size": ts,
                          "frame_bytes": nbytes // out.shape[0], "bytes_per_call": nbytes, "ms_median": round(med, 4),
                          "ms_min": round(min(ms), 4), "TB_per_s": round(nbytes / med / 1e9, 3), "bpc": args.bpc}), flush=True)
        del out
        env.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
