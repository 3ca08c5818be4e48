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


def piece_cells(np, ts):
    """float32[pieces, 49]: does 64-byte piece p of a frame hold a byte of view cell c (byte b = a colour of pixel b // 3 = (7 ts) y + x,
    which shows cell (x // ts) * 7 + y // ts)."""
    p = np.arange(147 * ts * ts) // 3
    cob = ((p % (7 * ts)) // ts * 7 + p // (7 * ts) // ts).reshape(-1, 64)
    m = np.zeros((len(cob), 49), np.float32)
    m[np.arange(len(cob))[:, None], cob] = 1
    return m


def delta_mode(args, np, torch, name):
    """Step BossLevel with bench.py's random actions and render every step into the registered target (what step() of a pixel batch of
    this tile size enqueues), the whole-frame render (option "render_delta" 0: k_view_pixels through the same call) and the delta render
    (1: k_view_delta) alternated in ONE process, --delta-reps repetitions of --delta-steps timed renders each; HIP-event time of the render
    call alone.  Next to it, on the frames of the timed steps, what tools/dirty_bytes.py's rule stores: the 64-byte pieces that hold a
    byte of a cell whose 3-byte encoding changed."""
    from babyai_amd.engine import BatchedBabyAIEnv, _check
    from babyai_amd.action_stream import actions_torch
    level, n, ts = WORKLOADS[name]
    dev = torch.device("cuda", 0)
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=dev, seeds=1, pixel=True, tile_size=ts)
    assert env.get_option("render_target_tile_size") == ts
    env.reset()
    pool = actions_torch(1234, 0, 64, 0, n, dev)
    pc = torch.as_tensor(piece_cells(np, ts), device=dev)
    frame = 147 * ts * ts
    t = [0]

    def step():
        act = pool[t[0] % 64]
        t[0] += 1
        _check(env.lib, env.lib.bbai_step(env.handle, act.data_ptr(), *env._step_out(), env._stream()), "bbai_step")

    def render():
        env._render_view_into(env.image, None, n, ts, env.pixels)

    for _ in range(16):
        step()
        render()
    per = {"full": [], "delta": []}
    rule_bytes, clean, frames = 0, 0, 0
    for rep in range(args.delta_reps):
        for mode in ("full", "delta"):
            env.set_option("render_delta", 1 if mode == "delta" else 0)
            for _ in range(3):                       # (the first render behind the switch draws whole frames and fills the shadow)
                step()
                render()
            assert env.get_option("render_delta_valid") == (1 if mode == "delta" else 0)
            ms = []
            for _ in range(args.delta_steps):
                prev = env.image.clone()
                step()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                render()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
                changed = (env.image != prev).reshape(n, 49, 3).any(dim=2)      # (the same work behind both modes' renders)
                rule_bytes += int(((changed.float() @ pc.t()) > 0).sum()) * 64
                clean += int((~changed.any(dim=1)).sum())
                frames += n
            per[mode].append(float(np.median(ms)))
            print(json.dumps({"workload": name, "rep": rep, "mode": mode, "ms_median": round(per[mode][-1], 4), "ms_min": round(min(ms), 4),
                              "ms_max": round(max(ms), 4)}), flush=True)
    full, delta = float(np.median(per["full"])), float(np.median(per["delta"]))
    spread = max(per["full"]) - min(per["full"])
    print(json.dumps({"workload": name, "level": level, "envs": n, "tile_size": ts, "frame_bytes": frame, "reps": args.delta_reps,
                      "steps_per_rep": args.delta_steps, "full_ms": [round(x, 4) for x in per["full"]], "delta_ms": [round(x, 4) for x in per["delta"]],
                      "full_ms_median": round(full, 4), "delta_ms_median": round(delta, 4), "full_spread_ms": round(spread, 4),
                      "delta_below_full_by_more_than_the_spread": bool(full - delta > spread), "delta_over_full": round(delta / full, 3),
                      "rule_bytes_per_frame": round(rule_bytes / max(frames, 1), 1), "rule_share_of_frame": round(rule_bytes / max(frames, 1) / frame, 4),
                      "clean_share": round(clean / max(frames, 1), 4)}), flush=True)
    env.close()
    torch.cuda.empty_cache()


def pmc_digest(path):
    """WRITE_SIZE per launch of the view kernels from a `rocprofv3 --pmc WRITE_SIZE` pass of `--delta` (counter_collection.csv; KB)."""
    import collections
    import csv
    import glob
    hits = sorted(glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True))
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(hits[0])):
        if r["Counter_Name"] == "WRITE_SIZE" and "k_view_" in r["Kernel_Name"]:
            agg[r["Kernel_Name"].split("(")[0].replace("void ", "")].append(float(r["Counter_Value"]))
    for k, v in sorted(agg.items()):
        v = sorted(v)
        print(json.dumps({"kernel": k, "launches": len(v), "WRITE_SIZE_KB_median": v[len(v) // 2], "min": v[0], "max": v[-1],
                          "mean": round(sum(v) / len(v), 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--no-grid", action="store_true", help="skip the k_render_grid comparison")
    ap.add_argument("--delta", action="store_true", help="the delta render into the registered target against the whole-frame render (delta_mode)")
    ap.add_argument("--delta-reps", type=int, default=4)
    ap.add_argument("--delta-steps", type=int, default=20)
    ap.add_argument("--pmc-digest", default=None, help="condense the counter_collection.csv under this directory and exit")
    args = ap.parse_args()
    if args.pmc_digest:
        return pmc_digest(args.pmc_digest)
    import numpy as np
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    if args.delta:
        for name in args.only.split(","):
            delta_mode(args, np, torch, name)
        return
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
