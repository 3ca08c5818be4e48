#!/usr/bin/env python3
"""The numbers of `DemoStore.collect_seeds` (GPU box; DESIGN.md section 5i quotes them).

    python tools/seed_demos_bench.py [--out profiles/seed_demos/seed_demos_bench.jsonl] [--boss 131072] [--local 65536] [--reps 2] [--reseed-levels 1]

One JSON line per measurement, the file rewritten on every run.  Per workload (BossLevel / GoToLocal, seeds 1000 ...) and look-ahead period
(the default, and BBAI_LOOKAHEAD=4), alternated `--reps` times in one process:
  collect_seeds at pool 8192, pool 32768 and pool = len(seeds) (one env per seed: no reseed), demos/s by the wall clock around the call;
  `DemoStore.collect` of the same seed range -- the outside reference: the same demonstrations where every first episode is solved.
The first repetition of every collect_seeds run also brackets the parts of its rounds by HIP events (imitation.ROUND_EVENTS): the share of
the summed round time spent in bot_rollout, reseed, k_demo_jobs, the pack and the extend.  A configuration whose history ring does not fit
half of the free device memory is reported with the error it raises.
--reseed-levels K: the POOL rows only (no one-env-per-seed run, no `collect`), each pool alternated without and with
collect_seeds(reseed_levels=K) -- short reseeds, the envs parking behind their K levels -- and the two results compared."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_demos", "seed_demos_bench.jsonl"))
    ap.add_argument("--boss", type=int, default=131072)
    ap.add_argument("--local", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--pools", default="8192,32768")
    ap.add_argument("--reseed-levels", type=int, default=None)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
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

    default_la = os.environ.pop("BBAI_LOOKAHEAD", None)
    for level, n in (("BabyAI-GoToLocal-v0", a.local), ("BabyAI-BossLevel-v0", a.boss)):
        if n <= 0:
            continue
        pools = [int(p) for p in a.pools.split(",") if int(p) < n] + [n]
        for lookahead in ("default", "4"):
            if lookahead == "default":
                os.environ.pop("BBAI_LOOKAHEAD", None)
            else:
                os.environ["BBAI_LOOKAHEAD"] = lookahead
            DemoStore.collect_seeds(level, range(1000, 1256), pool=64)          # warm-up: allocator, library, kernels
            variants = [(p, None) for p in pools + ["collect"]] if a.reseed_levels is None else [(p, k) for p in pools[:-1] for k in (None, a.reseed_levels)]
            for rep in range(a.reps):
                for path, depth in variants:
                    rec = dict(what="demos", level=level, seeds=n, lookahead=lookahead, rep=rep, path="collect" if path == "collect" else "collect_seeds",
                               pool=None if path == "collect" else path, one_env_per_seed=path == n, reseed_levels=depth)
                    imitation.ROUND_EVENTS = [] if (rep == 0 and path != "collect") else None
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    try:
                        if path == "collect":
                            store = DemoStore.collect(level, n, 1000, batch=n)
                            kept = len(store)
                        else:
                            store, k = DemoStore.collect_seeds(level, range(1000, 1000 + n), pool=path, reseed_levels=depth)
                            kept = len(k)
                            if a.reseed_levels is not None:          # the two variants return the same demonstrations
                                digest = (kept, store.num_frames, int(store.action.to(torch.int64).sum()), int(store.image[::97].to(torch.int64).sum()))
                                rec.update(digest=list(digest))
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        rec.update(seconds=dt, demos_per_s=kept / dt, seeds_per_s=n / dt, kept=kept, frames=store.num_frames)
                        del store
                    except (ValueError, RuntimeError) as exc:
                        rec.update(error=str(exc)[:300])
                    events, imitation.ROUND_EVENTS = imitation.ROUND_EVENTS, None
                    if events:
                        ms = {}
                        for part, e0, e1 in events:
                            ms[part] = ms.get(part, 0.0) + e0.elapsed_time(e1)
                        total = sum(ms.values())
                        rec.update(rounds=sum(1 for p, _, _ in events if p == "bot_rollout"), reseeds=sum(1 for p, _, _ in events if p == "reseed"),
                                   event_ms={k: round(v, 3) for k, v in ms.items()}, event_share={k: round(v / total, 4) for k, v in ms.items()})
                    emit(**rec)
                    torch.cuda.empty_cache()
    if default_la is not None:
        os.environ["BBAI_LOOKAHEAD"] = default_la
    out.close()


if __name__ == "__main__":
    main()
