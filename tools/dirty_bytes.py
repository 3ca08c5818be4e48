#!/usr/bin/env python3
"""tools/dirty_bytes.py -- how many bytes the delta render stores per env-step at each store granularity.

Replays the host oracle (oracle.levels) for --envs envs (seeds 1000 + i) over --steps steps of bench.py's action stream
(babyai_amd.action_stream.action_scalar(0, t, i)), with auto-reset, and diffs consecutive encoded views per cell: a cell is dirty
when its 3-byte encoding changes (the rule of the device's tile-id shadow).  A dirty cell's pixels are 8 rows of 24 bytes at a
168-byte pitch; for every unit P the P-aligned blocks of the flat frame buffer (env i at byte 9408 i) that cover them are counted.
Prints one JSON line: bytes per env-step for P = 128, 64, 32, 16 and for exactly the changed cell rows, and the share of clean
env-steps.

    python tools/dirty_bytes.py --level BossLevel --envs 256 --steps 60
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIX_BYTES, PITCH, VIEW = 9408, 168, 7
UNITS = (128, 64, 32, 16)


def cell_rows(cell):
    """(start byte, 24) of the 8 pixel rows of cell x * 7 + y inside an env's image."""
    x, y = divmod(cell, VIEW)
    return [(py * PITCH + x * 24) for py in range(8 * y, 8 * y + 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", default="BossLevel")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    from oracle import levels as olevels
    from babyai_amd.action_stream import action_scalar
    rows = [cell_rows(c) for c in range(VIEW * VIEW)]
    envs, obs = [], []
    for i in range(args.envs):
        env = olevels.make_env("BabyAI-%s-v0" % args.level)
        env.seed(1000 + i)
        envs.append(env)
        obs.append(env.reset()["image"].copy())
    stored = {P: 0 for P in UNITS}
    exact = clean = 0
    for t in range(args.steps):
        blocks = {P: set() for P in UNITS}
        for i, env in enumerate(envs):
            o, _, done, _ = env.step(action_scalar(0, t, i))
            if done:
                o = env.reset()
            new = o["image"]
            dirty = np.nonzero((new != obs[i]).any(axis=2).reshape(-1))[0]     # image[x][y] -> cell x * 7 + y
            obs[i] = new.copy()
            if len(dirty) == 0:
                clean += 1
            base = i * PIX_BYTES
            for c in dirty:
                for s in rows[c]:
                    exact += 24
                    for P in UNITS:
                        for b in range((base + s) // P, (base + s + 23) // P + 1):
                            blocks[P].add(b)
        for P in UNITS:
            stored[P] += len(blocks[P]) * P
    n = args.envs * args.steps
    out = {"level": args.level, "envs": args.envs, "steps": args.steps, "clean_share": round(clean / n, 4),
           "exact_bytes_per_env_step": round(exact / n, 1)}
    for P in UNITS:
        out["bytes_per_env_step_%d" % P] = round(stored[P] / n, 1)
        out["vs_exact_%d" % P] = round(stored[P] / max(exact, 1), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
