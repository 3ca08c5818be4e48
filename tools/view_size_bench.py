#!/usr/bin/env python3
"""Rate of the view-size observation (k_view_obs<V>; BatchedBabyAIEnv(view_size=V)): per workload and per V in 3, 5, 7, 9, 11, HIP-event
medians after warm-up of
  - observe_view(view_size=V) of every env (bbai_observe_view: the kernel alone),
  - a plain fill (torch fill_) of a buffer of the same 3 V^2 n bytes, alternated with it in the same process: the store rate the box gives
    a kernel that does nothing else,
  - step() with view_size=V (bbai_step_view: the step's launches + k_view_obs<V> as one call) and without (bbai_step) on twin batches,
    alternated call by call,
and the achieved rate on the algorithmic bytes of a frame: 3 V^2 stored + the V x V window bytes + the 16-byte Hot read per env.  (The
kernel stages V rows of (V + 6) / 4 aligned dwords, `staged_bytes_per_env`: what it really asks the memory system for.)  One JSON line per
(workload, V), to stdout and to --out.

    python tools/view_size_bench.py [--reps 30] [--only gotolocal,pickuploc,boss] [--sizes 3,5,7,9,11] [--out profiles/view_size/view_size_bench.jsonl]

Under `rocprofv3 --kernel-trace --stats` the same command gives the kernel's own time.
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


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--sizes", default="3,5,7,9,11")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    if not torch.cuda.is_available():
        raise SystemExit("view_size_bench needs the GPU: nothing is measured without one")
    sizes = [int(v) for v in args.sizes.split(",")]
    out = open(args.out, "a") if args.out else None
    dev = "cuda:0"
    for name in args.only.split(","):
        level, n = WORKLOADS[name]
        view = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=dev, seeds=1, view_size=sizes[0] if sizes[0] != 7 else 9)
        plain = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=dev, seeds=1)
        view.reset()
        plain.reset()
        rng = np.random.RandomState(0)
        acts = [torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=dev) for _ in range(16)]
        for V in sizes:
            frame = 3 * V * V
            buf = torch.zeros((n, V, V, 3), dtype=torch.uint8, device=dev)
            fill = torch.zeros((n * frame,), dtype=torch.uint8, device=dev)
            if V != 7:                        # the twin steps through bbai_step_view at this size: its view buffer is swapped per V
                view.view_size, view.view = V, buf
            for t in range(args.warmup):
                view.step(acts[t % 16])
                plain.step(acts[t % 16])
                view.observe_view(view_size=V, out=buf)
                fill.fill_(t)
            torch.cuda.synchronize()
            obs_ms, fill_ms, step_view, step_plain = [], [], [], []
            for r in range(args.reps):        # alternated: both see the same box state
                obs_ms.append(timed(torch, lambda: view.observe_view(view_size=V, out=buf)))
                fill_ms.append(timed(torch, lambda: fill.fill_(r)))
            for r in range(args.reps):
                if V != 7:
                    step_view.append(timed(torch, lambda: view.step(acts[r % 16])))
                step_plain.append(timed(torch, lambda: plain.step(acts[r % 16])))
            per_env = frame + V * V + 16
            algo = n * per_env
            med, fmed = float(np.median(obs_ms)), float(np.median(fill_ms))
            line = {"workload": name, "level": level, "envs": n, "view_size": V, "frame_bytes": frame, "algorithmic_bytes_per_env": per_env,
                    "staged_bytes_per_env": frame + 4 * V * ((V + 6) // 4) + 16, "algorithmic_bytes": algo,
                    "observe_view_ms_median": round(med, 4), "observe_view_ms_min": round(min(obs_ms), 4),
                    "TB_per_s_algorithmic": round(algo / med / 1e9, 3), "frac_of_8TBs": round(algo / med / 1e9 / PEAK_TBS, 3),
                    "fill_bytes": n * frame, "fill_ms_median": round(fmed, 4), "fill_TB_per_s": round(n * frame / fmed / 1e9, 3),
                    "stored_TB_per_s": round(n * frame / med / 1e9, 3), "store_rate_over_fill": round(fmed / med, 3),
                    "step_view_ms_median": round(float(np.median(step_view)), 4) if step_view else None,
                    "step_plain_ms_median": round(float(np.median(step_plain)), 4),
                    "step_view_minus_plain_ms": round(float(np.median(step_view)) - float(np.median(step_plain)), 4) if step_view else None,
                    "reps": args.reps}
            s = json.dumps(line)
            print(s, flush=True)
            if out:
                out.write(s + "\n")
                out.flush()
            del buf, fill
        assert view.gate_timeouts() == 0 and plain.gate_timeouts() == 0
        view.close()
        plain.close()
        del view, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
