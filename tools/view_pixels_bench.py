#!/usr/bin/env python3
"""Rate of the partial-view picture at any view size (k_view_pixels_n<V, TS>; include/bbai_view_pixels.h bbai_render_view_pixels;
BatchedBabyAIEnv.render_encoding / render_view with view_size=V): per workload, per V in 3, 5, 7, 9, 11 and per tile size 8, 16, 32,
HIP-event medians after warm-up of
  - the kernel alone: bbai_render_view_pixels of `count` rows of a RESIDENT encoded buffer uint8[count, V, V, 3] (observe_view's frames
    of the stepped batch, taken once),
  - render_view(ids, tile_size, view_size=V) from the state: observe_view into a scratch encoding + the same launch,
  - a plain fill (torch fill_) of the same output buffer, alternated with each in the same process: the store rate the box gives a
    kernel that does nothing else.
`count` is the workload's batch size (DESIGN section 5l's table), halved until count x frame bytes fits a quarter of the free device
memory (`envs` / `count` in every line say which cases were reduced).  One JSON line per (workload, V, tile size), to stdout and --out.

    python tools/view_pixels_bench.py [--reps 30] [--only gotolocal,pickuploc,boss] [--sizes 3,5,7,9,11] [--tiles 8,16,32] [--out profiles/view_pixels/view_pixels_n_bench.jsonl]

--ab7: the new kernel against the 7x7 kernels instead, alternated call by call in one process, each into an unregistered buffer of
about 9.9 GB of frames: bbai_render_view at tile sizes 16 / 32 (262 144 / 65 536 rows), bbai_render on the full batch at 8 (1 048 576
rows); one line per tile size with both medians, their ratio and each side's own spread (quartiles, min, max).

Under `rocprofv3 --kernel-trace --stats` the same command gives the kernels' own times.
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


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(np, xs):
    q = np.percentile(xs, [25, 50, 75])
    return {"median": round(float(q[1]), 4), "p25": round(float(q[0]), 4), "p75": round(float(q[2]), 4), "min": round(float(min(xs)), 4),
            "max": round(float(max(xs)), 4)}


def emit(out, line):
    s = json.dumps(line)
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


def stepped_batch(np, torch, level, n, dev, steps=6, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=dev, seeds=1, **kw)
    env.reset()
    rng = np.random.RandomState(0)
    for _ in range(steps):
        env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=dev))
    return env


def bench(args, np, torch, out):
    from babyai_amd import engine
    dev = "cuda:0"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [int(v) for v in args.sizes.split(",")]
    tiles = [int(t) for t in args.tiles.split(",")]
    for name in args.only.split(","):
        level, n = WORKLOADS[name]
        env = stepped_batch(np, torch, level, n, dev)
        for V in sizes:
            resident = env.observe_view(view_size=V).clone()              # uint8[n, V, V, 3]
            for ts in tiles:
                frame = 3 * V * V * ts * ts
                torch.cuda.empty_cache()
                free = torch.cuda.mem_get_info(0)[0]
                count = n
                while count * frame > free // 4:
                    count //= 2
                buf = torch.empty((count, V * ts, V * ts, 3), dtype=torch.uint8, device=dev)
                ids = None if count == n else torch.arange(count, dtype=torch.int64, device=dev)
                enc = resident[:count]

                def kernel():
                    env._view_pixels_into(enc, None, count, V, ts, buf)

                def from_state():
                    env.render_view(ids, tile_size=ts, out=buf, view_size=V) if V != 7 else \
                        env._view_pixels_into(env.observe_view(ids, 7), None, count, 7, ts, buf)
                for t in range(args.warmup):
                    kernel()
                    from_state()
                    buf.fill_(t)
                torch.cuda.synchronize()
                k_ms, kf_ms, s_ms, sf_ms = [], [], [], []
                for r in range(args.reps):        # alternated: both see the same box state
                    k_ms.append(timed(torch, kernel))
                    kf_ms.append(timed(torch, lambda: buf.fill_(r)))
                for r in range(args.reps):
                    s_ms.append(timed(torch, from_state))
                    sf_ms.append(timed(torch, lambda: buf.fill_(r)))
                k, kf, s, sf = (float(np.median(x)) for x in (k_ms, kf_ms, s_ms, sf_ms))
                epi, slices, items, blocks = engine.view_pixels_items(V, ts, count, cus)
                emit(out, {"workload": name, "level": level, "envs": n, "count": count, "reduced": count != n, "view_size": V, "tile_size": ts,
                           "frame_bytes": frame, "bytes": count * frame, "envs_per_item": epi, "slices": slices, "items": items, "blocks": blocks,
                           "kernel_ms_median": round(k, 4), "kernel_ms_min": round(min(k_ms), 4), "kernel_TB_per_s": round(count * frame / k / 1e9, 3),
                           "fill_ms_median": round(kf, 4), "fill_TB_per_s": round(count * frame / kf / 1e9, 3), "store_rate_over_fill": round(kf / k, 3),
                           "render_view_ms_median": round(s, 4), "render_view_fill_ms_median": round(sf, 4),
                           "render_view_rate_over_fill": round(sf / s, 3), "reps": args.reps})
                del buf
            del resident
        assert env.gate_timeouts() == 0
        env.close()
        del env
        torch.cuda.empty_cache()


def ab7(args, np, torch, out):
    dev = "cuda:0"
    n = 1048576
    env = stepped_batch(np, torch, "BossLevel", n, dev)                   # (an encoded batch: no registered target)
    for ts in (int(t) for t in args.tiles.split(",")):
        count = n * 64 // (ts * ts)
        enc = env.image[:count]
        buf = torch.empty((count, 7 * ts, 7 * ts, 3), dtype=torch.uint8, device=dev)
        env._install_atlas("view", ts)

        def old():
            env.render_encoding(enc, out=buf, tile_size=ts)               # bbai_render (8: the full batch) / bbai_render_view (16, 32)

        def new():
            env._view_pixels_into(enc, None, count, 7, ts, buf)
        for t in range(args.warmup):
            old()
            new()
            buf.fill_(t)
        torch.cuda.synchronize()
        o_ms, n_ms, f_ms = [], [], []
        for r in range(args.reps):
            o_ms.append(timed(torch, old))
            n_ms.append(timed(torch, new))
            f_ms.append(timed(torch, lambda: buf.fill_(r)))
        so, sn, sf = spread(np, o_ms), spread(np, n_ms), spread(np, f_ms)
        emit(out, {"ab": "view_size_7", "tile_size": ts, "rows": count, "bytes": count * 147 * ts * ts,
                   "existing": "bbai_render" if ts == 8 else "bbai_render_view", "existing_ms": so, "view_pixels_n_ms": sn, "fill_ms": sf,
                   "new_over_existing": round(sn["median"] / so["median"], 4),
                   "existing_spread_rel": round((so["p75"] - so["p25"]) / so["median"], 4),
                   "new_spread_rel": round((sn["p75"] - sn["p25"]) / sn["median"], 4), "reps": args.reps})
        del buf
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--sizes", default="3,5,7,9,11")
    ap.add_argument("--tiles", default="8,16,32")
    ap.add_argument("--ab7", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("view_pixels_bench needs the GPU: nothing is measured without one")
    out = open(args.out, "a") if args.out else None
    (ab7 if args.ab7 else bench)(args, np, torch, out)


if __name__ == "__main__":
    main()
