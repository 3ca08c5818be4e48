#!/usr/bin/env python3
"""The numbers of `DemoStore.replay` (GPU box; DESIGN.md section 5k quotes them).

    python tools/demo_replay_bench.py [--out profiles/demo_replay/demo_replay_bench.jsonl] [--local 262144] [--boss 196608] [--reps 3]

One JSON line per measurement, the file rewritten on every run.  Per workload (GoToLocal / BossLevel, seeds 1000 ...): a store collected
with `DemoStore.collect_seeds`, then replayed at pools 4 096 / 32 768 / 131 072 and reseed_every 1 / 4 / 16, the nine configurations
alternated `--reps` times in one process behind a warm-up replay of every pool size.  Per run: demos/s and frames/s by the wall clock around
the call (which ends in the loop's last counter read), whether every demo came back exact, and -- on the first repetition, which is not the
one to quote the rates from -- the parts of its ticks bracketed by HIP events (imitation.ROUND_EVENTS): the summed time of feed, step (the
bare bbai_step under HOLD bytes), judge and reseed, and (feed + judge) / step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOLS = (4096, 32768, 131072)
EVERY = (1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demo_replay", "demo_replay_bench.jsonl"))
    ap.add_argument("--local", type=int, default=262144)
    ap.add_argument("--boss", type=int, default=196608)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pools", default=",".join(str(p) for p in POOLS))
    ap.add_argument("--every", default=",".join(str(r) for r in EVERY))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import numpy as np
    import torch
    from babyai_amd import imitation
    from babyai_amd.imitation import DemoStore
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, "w")

    def emit(**rec):
        line = json.dumps(rec, sort_keys=True)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    pools, every = [int(p) for p in a.pools.split(",")], [int(r) for r in a.every.split(",")]
    for level, n in (("BabyAI-GoToLocal-v0", a.local), ("BabyAI-BossLevel-v0", a.boss)):
        if n <= 0:
            continue
        seeds = np.arange(1000, 1000 + n, dtype=np.uint64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store, kept = DemoStore.collect_seeds(level, seeds, pool=min(n, 32768), reseed_levels=1)
        torch.cuda.synchronize()
        emit(what="collect", level=level, seeds=n, kept=len(kept), frames=store.num_frames, seconds=time.perf_counter() - t0)
        seeds = seeds[kept]
        for p in pools:                         # warm-up: allocator, library, kernels, every pool size
            store.replay(level, seeds, pool=p)
        for rep in range(a.reps):
            for p in pools:
                for r in every:
                    rec = dict(what="replay", level=level, demos=len(store), frames=store.num_frames, pool=min(p, len(store)), reseed_every=r, rep=rep)
                    imitation.ROUND_EVENTS = [] if rep == 0 else None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = store.replay(level, seeds, pool=p, reseed_every=r)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    events, imitation.ROUND_EVENTS = imitation.ROUND_EVENTS, None
                    rec.update(seconds=dt, demos_per_s=len(store) / dt, frames_per_s=store.num_frames / dt, exact=int(res.exact.sum()), timed_by_events=bool(events))
                    if events:
                        ms = {}
                        for part, e0, e1 in events:
                            ms[part] = ms.get(part, 0.0) + e0.elapsed_time(e1)
                        rec.update(ticks=sum(1 for part, _, _ in events if part == "step"), reseeds=sum(1 for part, _, _ in events if part == "reseed"),
                                   event_ms={k: round(v, 3) for k, v in ms.items()},
                                   feed_judge_over_step=round((ms.get("feed", 0.0) + ms.get("judge", 0.0)) / ms["step"], 4))
                    emit(**rec)
                    del res
        del store
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
