#!/usr/bin/env python3
"""step() of a full_obs pixel batch (RGBImgObsWrapper: BatchedBabyAIEnv(full_obs=True, pixel=True, tile_size=ts)) under the action stream's
random actions (babyai_amd/action_stream.py), HIP events around every step after warm-up: median and quartiles per workload.  With the
registered full-grid target (include/bbai_grid_target.h) a step stores only the 64-byte pieces that changed (k_grid_delta); a library
without the entries -- the parent's, BBAI_ENGINE_LIB -- draws every frame whole (k_render_grid), which is the baseline.

    python tools/grid_delta_bench.py [--only boss8,local8,local16,boss32] [--steps 60] [--out FILE]         one process, this library
    python tools/grid_delta_bench.py --pairs 3 --parent-lib parent.so --out profiles/grid_delta/ab.jsonl    fresh processes, parent / this build alternated
    python tools/grid_delta_bench.py --inprocess --out ...      option "grid_render_delta" 1 against 0, alternated block by block inside one process
    python tools/grid_delta_bench.py --share --out ...          the share of a frame's bytes a step stores, counted on 1 024 envs: the registered
                                                                 buffer is overwritten with 255 - (the new frame) before a delta render, and the
                                                                 bytes that then hold the new frame are the ones stored

A workload whose frames do not fit a quarter of the free device memory is halved until they do (the line says so: "envs" against "envs_asked").
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "boss8": ("BossLevel", 131072, 8),
    "local8": ("GoToLocal", 65536, 8),
    "local16": ("GoToLocal", 65536, 16),
    "boss32": ("BossLevel", 16384, 32),
}
SHARE_ENVS = 1024


def quartiles(np, ms):
    q1, med, q3 = (float(v) for v in np.percentile(np.asarray(ms), [25, 50, 75]))
    return {"ms_median": round(med, 4), "ms_q1": round(q1, 4), "ms_q3": round(q3, 4), "ms_min": round(float(min(ms)), 4)}


def fitting(torch, level, n, ts):
    from babyai_amd.levels import make_cfg
    c = make_cfg("BabyAI-%s-v0" % level)
    frame = 3 * c.W * c.H * ts * ts
    free = torch.cuda.mem_get_info(0)[0]
    asked = n
    while n > 1 and n * frame > free // 4:
        n //= 2
    return n, asked, frame


def timed_steps(torch, env, pool, steps, t0=0):
    ms = []
    for t in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        env.step(pool[(t0 + t) % len(pool)])
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def make(level, n, ts):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device="cuda:0", seeds=1, pixel=True, full_obs=True, tile_size=ts)
    env.reset()
    return env


def run_plain(args, emit):
    import numpy as np
    import torch
    from babyai_amd.action_stream import actions_torch
    for name in args.only.split(","):
        level, n, ts = WORKLOADS[name]
        n, asked, frame = fitting(torch, level, n, ts)
        env = make(level, n, ts)
        pool = actions_torch(1234, 0, 64, 0, n, torch.device("cuda", 0))
        timed_steps(torch, env, pool, args.warmup)
        torch.cuda.synchronize()
        rec = {"workload": name, "level": level, "envs": n, "envs_asked": asked, "tile_size": ts, "frame_bytes": frame, "steps": args.steps,
               "library": os.path.basename(os.environ.get("BBAI_ENGINE_LIB", "")) or "this build", "grid_target": bool(env._grid_target)}
        if args.inprocess and env._grid_target:
            ms = {1: [], 0: []}
            for blk in range(args.steps // 10):        # alternated block by block: both settings see the same box state
                for opt in (1, 0):
                    env.set_option("grid_render_delta", opt)
                    env.step(pool[0])                   # (the first step behind a switch is not timed)
                    ms[opt] += timed_steps(torch, env, pool, 10, 1 + 10 * blk)
            env.set_option("grid_render_delta", 1)
            rec.update({"delta_" + k: v for k, v in quartiles(np, ms[1]).items()})
            rec.update({"whole_" + k: v for k, v in quartiles(np, ms[0]).items()})
        else:
            rec.update(quartiles(np, timed_steps(torch, env, pool, args.steps, args.warmup)))
        emit(rec)
        env.close()
        del env
        torch.cuda.empty_cache()


def run_share(args, emit):
    import torch
    from babyai_amd.action_stream import actions_torch
    for name in args.only.split(","):
        level, _, ts = WORKLOADS[name]
        n = SHARE_ENVS
        env = make(level, n, ts)
        if not env._grid_target:
            raise SystemExit("--share needs a library with the grid target entries")
        pool = actions_torch(1234, 0, 64, 0, n, torch.device("cuda", 0))
        stored = total = pieces = 0
        for t in range(args.steps):
            rc = env.lib.bbai_step(env.handle, ctypes.c_void_p(pool[t % 64].data_ptr()), *env._step_out(), env._stream())
            if rc != 0:
                raise SystemExit("bbai_step failed (%d)" % rc)
            new = env.render_grid(None, tile_size=ts, highlight=False)
            env.full.copy_(255 - new)
            env.observe_full()                          # the delta render: what now holds the new frame was stored
            hit = (env.full == new).view(n, -1, 64)
            if not bool((hit.all(dim=2) | ~hit.any(dim=2)).all()):
                raise SystemExit("a 64-byte piece was stored in part")
            p = hit.all(dim=2)
            stored += int(p.sum()) * 64
            pieces += int(p.sum())
            total += new.numel()
            env.full.copy_(new)
        emit({"share": name, "level": level, "envs": n, "tile_size": ts, "steps": args.steps, "stored_bytes_per_env_step": round(stored / (n * args.steps), 1),
              "stored_share": round(stored / total, 6), "pieces_per_env_step": round(pieces / (n * args.steps), 3)})
        env.close()
        del env
        torch.cuda.empty_cache()


def run_pairs(args, emit):
    import numpy as np
    if not args.parent_lib or not os.path.isfile(args.parent_lib):
        raise SystemExit("--pairs needs --parent-lib: the parent commit's library")
    got = {}
    for p in range(1, args.pairs + 1):
        for who in (("parent", "this") if p % 2 else ("this", "parent")):
            e = dict(os.environ)
            e.pop("BBAI_ENGINE_LIB", None)
            if who == "parent":
                e["BBAI_ENGINE_LIB"] = os.path.abspath(args.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", args.only, "--steps", str(args.steps), "--warmup", str(args.warmup)],
                                 cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.run_timeout)
            text = out.stdout.decode(errors="replace")
            if out.returncode != 0:
                sys.stderr.write(text[-4000:])
                raise SystemExit("%s run %d ended with status %d -- nothing more is started" % (who, p, out.returncode))
            for line in text.splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    rec["run"] = "%s_%d" % (who, p)
                    emit(rec)
                    got.setdefault((rec["workload"], who), []).append(rec["ms_median"])
    for name in args.only.split(","):
        par, this = got[(name, "parent")], got[(name, "this")]
        emit({"summary": name, "pairs": args.pairs, "parent_median_ms": round(float(np.median(par)), 4), "parent_spread_ms": round(max(par) - min(par), 4),
              "this_build_median_ms": round(float(np.median(this)), 4), "this_build_spread_ms": round(max(this) - min(this), 4),
              "speedup": round(float(np.median(par)) / float(np.median(this)), 2),
              "faster_by_more_than_parent_spread": bool(float(np.median(par)) - float(np.median(this)) > max(par) - min(par))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inprocess", action="store_true")
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--run-timeout", type=float, default=300.0, help="seconds one child run may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if args.out:                                     # (kept current: a run that stops early leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("".join(json.dumps(r) + "\n" for r in lines))

    if args.pairs:
        run_pairs(args, emit)
    elif args.share:
        run_share(args, emit)
    else:
        run_plain(args, emit)


if __name__ == "__main__":
    main()
