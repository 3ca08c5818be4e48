#!/usr/bin/env python3
"""Cost of stepping only the listed envs (include/bbai.h BBAI_ACTION_HOLD, option "step_hold"; BatchedBabyAIEnv.step(ids=...)), and what the
hold path costs the judged workload.  One JSON line per figure.

Part (a), one process: per workload the HIP-event time per call, on warm shapes and over at least --min-seconds of back-to-back calls
(three such batches, median first in `runs`), of
    step            the plain step() of the handle, every env stepping
    ids_64 / ids_4096 / ids_all
                    step(ids=...) with that many scattered envs listed (device id list): the binding's own launches included (the scatter of the
                    listed actions into the hold vector and its restore: three small launches)
    native_64 / native_4096 / native_all
                    the same hold vectors handed to step() directly with the option on: the native call alone
With --plain-only (a run against another library, BBAI_ENGINE_LIB: the parent's has no hold action) only `step` is measured; --parent-file
names that run's output, and every figure of the main run gets its ratio to the parent's full step at the same shape.

Part (b), --headline PAIRS --parent-lib PATH: the judged command `python bench.py --steps 20 --warmup 5`, one process per run, the parent's
library (BBAI_ENGINE_LIB) and this build alternated PAIRS times (the order inside a pair flips from pair to pair; --strict: parent first in
every pair, so that no run follows a run of its own library); a summary line with both medians, their difference and the parent's own
run-to-run spread (max - min of its runs), inside which the difference has to lie.

    python tools/step_hold_bench.py [--only boss,local] [--out profiles/step_hold/step_hold_bench.jsonl]
    BBAI_ENGINE_LIB=parent.so python tools/step_hold_bench.py --plain-only --out profiles/step_hold/parent_step.jsonl
    python tools/step_hold_bench.py --headline 6 --parent-lib parent.so --out profiles/step_hold/ab_headline.jsonl
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: level, envs in the batch
WORKLOADS = {
    "boss": ("BossLevel", 1048576),
    "local": ("GoToLocal", 65536),
}
LISTS = (64, 4096, None)        # None: every env listed
HEADLINE = ["bench.py", "--steps", "20", "--warmup", "5"]


def event_ms(torch, call, min_seconds, repeats=3):
    """ms per call: `repeats` timed batches of back-to-back calls, each at least min_seconds long; (median, all, calls per batch)."""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); call(); b.record(); b.synchronize()
    reps = max(1, int(min_seconds * 1e3 / max(a.elapsed_time(b), 1e-3)) + 1)
    runs = []
    for _ in range(repeats):
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) / reps)
    return sorted(runs)[len(runs) // 2], runs, reps


def part_a(args, emit):
    import numpy as np
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    dev = "cuda:0"
    parent = {}
    if args.parent_file:
        with open(args.parent_file) as f:
            for line in f:
                rec = json.loads(line)
                if rec.get("what") == "step":
                    parent[rec["workload"]] = rec["ms"]
    for name in args.only.split(","):
        level, n = WORKLOADS[name]
        env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=dev, seeds=1)
        env.reset()
        rng = np.random.RandomState(0)
        acts = torch.as_tensor(rng.randint(0, 7, size=(16, n)).astype(np.uint8), device=dev)
        turn = [0]

        def full():
            turn[0] = (turn[0] + 1) % 16
            return acts[turn[0]]

        for _ in range(8):
            env.step(full())

        def figure(what, call, listed):
            ms, runs, reps = event_ms(torch, call, args.min_seconds)
            rec = {"workload": name, "level": level, "envs": n, "what": what, "listed": listed, "ms": ms, "runs": sorted(runs), "calls_per_run": reps,
                   "library": os.path.basename(os.environ.get("BBAI_ENGINE_LIB", "")) or "this build"}
            if name in parent:
                rec["parent_step_ms"] = parent[name]
                rec["ratio_to_parent_step"] = ms / parent[name]
            emit(rec)

        figure("step", lambda: env.step(full()), n)
        if args.plain_only:
            env.close()
            continue
        for k in LISTS:
            ids = np.arange(n) if k is None else np.sort(rng.choice(n, size=k, replace=False))
            tag = "all" if k is None else str(k)
            ids_t = torch.as_tensor(ids, device=dev)
            figure("ids_" + tag, lambda: env.step(full()[:len(ids)], ids=ids_t), len(ids))
            vec = torch.full((n,), env.HOLD, dtype=torch.uint8, device=dev)
            vec[ids_t] = acts[0][ids_t]
            env.set_option("step_hold", 1)
            figure("native_" + tag, lambda: env.step(vec), len(ids))
            env.set_option("step_hold", 0)
        figure("step_again", lambda: env.step(full()), n)        # the first figure once more: what the visit's drift is
        assert env.gate_timeouts() == 0
        env.close()


def part_b(args, emit):
    def run(tag, lib):
        e = dict(os.environ)
        e.pop("BBAI_ENGINE_LIB", None)
        if lib:
            e["BBAI_ENGINE_LIB"] = os.path.abspath(lib)
        out = subprocess.run([sys.executable] + HEADLINE, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.run_timeout)
        text = out.stdout.decode(errors="replace")
        if out.returncode != 0:
            sys.stderr.write(text[-4000:])
            raise SystemExit("%s: bench.py ended with status %d -- nothing more is started" % (tag, out.returncode))
        res = None
        for line in text.splitlines():
            if line.startswith("{"):
                try:
                    res = json.loads(line)
                except ValueError:
                    pass
        rec = {"run": tag, "value": res.get("value"), "ms_per_step": res.get("ms_per_step")}
        if rec["ms_per_step"] is None and res.get("value"):
            rec["ms_per_step"] = res.get("envs", 1048576) / res["value"] * 1e3
        emit(rec)
        return rec["ms_per_step"]

    ms = {"parent": [], "this": []}
    for p in range(1, args.headline + 1):
        order = ("parent", "this") if p % 2 or args.strict else ("this", "parent")
        for who in order:
            ms[who].append(run("ab_%s_%d" % (who, p), args.parent_lib if who == "parent" else None))
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else sum(sorted(v)[len(v) // 2 - 1:len(v) // 2 + 1]) / 2
    spread = max(ms["parent"]) - min(ms["parent"])
    diff = med(ms["this"]) - med(ms["parent"])
    emit({"summary": "headline", "command": "python " + " ".join(HEADLINE), "pairs": args.headline, "parent_median": med(ms["parent"]), "parent_spread": spread,
          "this_build_median": med(ms["this"]), "this_build_spread": max(ms["this"]) - min(ms["this"]), "difference": diff, "inside_parent_spread": abs(diff) <= spread})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent-file", default=None)
    ap.add_argument("--headline", type=int, default=0, metavar="PAIRS")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--strict", action="store_true", help="--headline: parent, this, parent, this, ... (default: the order inside a pair flips from pair to pair)")
    ap.add_argument("--run-timeout", type=float, default=240.0, help="seconds one bench.py run may take")
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

    if args.headline:
        if not args.parent_lib or not os.path.isfile(args.parent_lib):
            raise SystemExit("--headline needs --parent-lib: the parent commit's library")
        part_b(args, emit)
    else:
        part_a(args, emit)


if __name__ == "__main__":
    main()
