#!/usr/bin/env python3
"""tools/render_delta_mix.py -- what delta rendering saves under two action mixes, settings alternated inside ONE process.

The delta render (include/bbai.h bbai_set_render_target) stores only the 128-byte lines whose cells changed, so its time depends on
the actions: a turn redraws most of the view, a blocked move or an object action almost nothing.  bench.py steps with uniform random
actions; a trained policy turns and moves more often than that.  The device expert (bbai_bot_act, k_bot) gives such a mix.  For each
mix, each repetition alternates render_delta 0 / 1 on one batch: a few untimed steps after the switch (the first render after it
writes every byte), then --steps steps with every k_step / k_render launch bracketed by events (bbai_profile).  One JSON line per
(mix, repetition, setting), then a summary line: median k_render ms per launch and the expert mix's action shares.

    python tools/render_delta_mix.py --envs 1048576 --steps 20 --reps 3
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", default="BossLevel")
    ap.add_argument("--envs", type=int, default=1048576)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    from babyai_amd.action_stream import actions_torch

    dev = torch.device("cuda:0")
    n = args.envs
    summary = {}
    for mix in ("random", "expert"):
        env = BatchedBabyAIEnv("BabyAI-%s-v0" % args.level, n, device=dev, pixel=True, seeds=args.seed)
        env.reset()
        t = [0]
        hist = torch.zeros(8, dtype=torch.int64, device=dev)

        def act():
            if mix == "random":
                a = actions_torch(args.seed + 1, t[0], t[0] + 1, 0, n, dev)[0]
            else:
                a = env.bot_actions()
                a = torch.where(a > 6, torch.full_like(a, 6), a)       # (a bot that gave up: the done action)
                hist.add_(torch.bincount(a.long(), minlength=8)[:8])
            t[0] += 1
            return a

        for _ in range(args.settle):
            env.step(act())
        for rep in range(args.reps):
            for delta in (0, 1):
                env.set_option("render_delta", delta)
                for _ in range(args.settle):
                    env.step(act())
                torch.cuda.synchronize()
                env.profile(True)
                for _ in range(args.steps):
                    env.step(act())
                torch.cuda.synchronize()
                k = env.profile_read()
                env.profile(False)
                rec = {"mix": mix, "rep": rep, "render_delta": delta, "envs": n, "steps": args.steps,
                       "k_render_ms": k["k_render"][0], "k_step_ms": k["k_step"][0]}
                summary.setdefault((mix, delta), []).append(rec["k_render_ms"])
                print(json.dumps(rec), flush=True)
        if mix == "expert":
            h = hist.cpu().tolist()
            tot = float(sum(h)) or 1.0
            summary["expert_action_shares"] = {name: round(h[i] / tot, 4) for i, name in enumerate(("left", "right", "forward", "pickup", "drop", "toggle", "done"))}
        env.close()
        del env
        torch.cuda.empty_cache()
    out = {"summary": True, "level": args.level, "envs": n,
           "k_render_ms_median": {"%s/render_delta=%d" % k: median(v) for k, v in summary.items() if isinstance(k, tuple)},
           "expert_action_shares": summary.get("expert_action_shares")}
    for mix in ("random", "expert"):
        full, delta = median(summary[(mix, 0)]), median(summary[(mix, 1)])
        out["speedup_%s" % mix] = round(full / delta, 3) if delta else None
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
