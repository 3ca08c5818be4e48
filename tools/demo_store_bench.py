#!/usr/bin/env python3
"""The demo store's numbers (GPU box; DESIGN.md section 5d quotes them).

    python tools/demo_store_bench.py [--parts demos,kernels,epoch] [--out profiles/demo_store/demo_store_bench.jsonl] [--streams 131072]

One JSON line per measurement, the file rewritten on every run:
  demos    demos/s of `DemoStore.collect` against `generate_demos`, alternated, at the sizes DESIGN.md section 8 row 4 quotes
  kernels  ONE launch of k_demo_pack and of k_demo_batch by HIP events, everything the launch needs prepared beforehand, on a BossLevel
           store far above the 256 MiB Infinity Cache (131 072 streams: 1.6 GB of images), beside `Tensor.copy_` of the same bytes in
           the same process.  `rocprofv3 --kernel-trace --stats -- python tools/demo_store_bench.py --parts kernels --out /dev/null`
           names the kernels' own times; counters (--pmc FETCH_SIZE / WRITE_SIZE) go in runs of their own
  epoch    frames/s of `run_epoch` (training, recurrence 20, batches of 256 demos) with a small recurrent model: a host-bound
           figure on a shared box
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demo_store", "demo_store_bench.jsonl"))
    ap.add_argument("--parts", default="demos,kernels,epoch")
    ap.add_argument("--streams", type=int, default=131072)
    a = ap.parse_args()
    parts = a.parts.split(",")
    import __graft_entry__ as g
    g.build()
    import torch
    from babyai_amd import imitation
    from babyai_amd.demos import generate_demos
    from babyai_amd.engine import BatchedBabyAIEnv, _check, load_library
    from babyai_amd.imitation import DemoStore
    if os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, "w")
    dev = torch.device("cuda:0")
    lib = load_library()

    def emit(**rec):
        line = json.dumps(rec, sort_keys=True)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps=5):
        """milliseconds of fn() on the stream, by events: (best, median) of `reps` after one warm-up"""
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]))
        return min(ms), sorted(ms)[len(ms) // 2]

    if "demos" in parts:
        for level, n in [("BabyAI-BossLevel-v0", 131072), ("BabyAI-BossLevel-v0", 32768), ("BabyAI-GoToLocal-v0", 65536)]:
            for rep in range(2):
                for path in ("collect", "generate_demos"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if path == "collect":
                        frames = DemoStore.collect(level, n, 1000, batch=n).num_frames
                    else:
                        frames = sum(len(d[3]) for d in generate_demos(level, n, 1000, batch=n))
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    emit(what="demos", path=path, level=level, streams=n, rep=rep, seconds=dt, demos_per_s=n / dt, frames=frames)

    if "kernels" in parts:
        # the history of one batch of streams, kept: what DemoStore.collect holds when it calls k_demo_pack
        level, n = "BabyAI-BossLevel-v0", a.streams
        env = BatchedBabyAIEnv(level, n, device=dev, seeds=[1000 + k for k in range(n)], auto_reset=True)
        env.enable_instr_tokens()
        env.reset()
        chunk = max(1, min(128, max(16, env.max_steps_bound // 4)))
        last = torch.full((n,), -1, dtype=torch.int32, device=dev)
        open_ = torch.ones(n, dtype=torch.uint8, device=dev)
        span = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        hist, g0, still = [], 0, n
        while still:
            r = env.bot_rollout(chunk, tokens=True)
            hist.append(r)
            imitation.demo_spans(r["done"], r["gave_up"], r["reward"], g0, 0, last, open_, span, counter)
            still = int(counter.item())
            g0 += chunk
        offset = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum((span[:, 1] - span[:, 0] + 1).to(torch.int64), 0, out=offset[1:])
        frames = int(offset[-1].item())
        table = torch.as_tensor(np.array([[r[k].data_ptr() for k in ("image", "direction", "action", "tokens")] for r in hist], dtype=np.int64), device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        image, direction, action = torch.empty((frames, 7, 7, 3), **u8), torch.empty(frames, **u8), torch.empty(frames, **u8)
        tokens = torch.empty((n, 72), **u8)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def pack():
            _check(lib, lib.bbai_demo_pack(n, frames, chunk, table.data_ptr(), span.data_ptr(), offset.data_ptr(), image.data_ptr(),
                                           direction.data_ptr(), action.data_ptr(), tokens.data_ptr(), stream), "bbai_demo_pack")
        pack_ms = timed(pack)
        store = DemoStore(image, direction, action, tokens, offset.cpu().numpy())
        del hist, table
        env.close()
        # the batch gather of the WHOLE store in shuffled order: order / starts on the device before the clock starts
        perm = np.random.default_rng(0).permutation(n)
        lens = store.lengths[perm]
        rank = np.argsort(-lens, kind="stable")
        order = torch.as_tensor(perm[rank], device=dev)
        start = torch.as_tensor(np.concatenate([[0], np.cumsum(lens[rank])]).astype(np.int64), device=dev)
        o_img = torch.empty_like(image)
        o_act, o_ep = torch.empty(frames, dtype=torch.int64, device=dev), torch.empty(frames, dtype=torch.int64, device=dev)
        o_done, o_mask = torch.empty(frames, dtype=torch.bool, device=dev), torch.empty((frames, 1), dtype=torch.float32, device=dev)

        def batch():
            _check(lib, lib.bbai_demo_batch(n, frames, order.data_ptr(), start.data_ptr(), store.offset.data_ptr(), image.data_ptr(), direction.data_ptr(),
                                            action.data_ptr(), o_img.data_ptr(), o_act.data_ptr(), o_done.data_ptr(), o_mask.data_ptr(), o_ep.data_ptr(),
                                            None, None, stream), "bbai_demo_batch")
        batch_ms = timed(batch)
        copy_ms = timed(lambda: o_img.copy_(image))
        img_bytes = frames * 147
        # bytes a launch must move at least: pack reads and writes every frame's 149 bytes once (+ 72 B of tokens per demo, both ways);
        # batch reads 148 B per frame (image + action) and writes 147 + 8 + 1 + 4 + 8
        pack_bytes = 2 * (frames * 149 + n * 72)
        batch_bytes = frames * (148 + 168)
        for name, ms, nbytes in (("k_demo_pack", pack_ms, pack_bytes), ("k_demo_batch", batch_ms, batch_bytes), ("copy_", copy_ms, 2 * img_bytes)):
            emit(what="kernel", kernel=name, level=level, streams=n, frames=frames, image_bytes=img_bytes, bytes_moved=nbytes, ms_best=ms[0], ms_median=ms[1],
                 GBps_best=nbytes / ms[0] / 1e6, fraction_of_copy_rate=(nbytes / ms[0]) / (2 * img_bytes / copy_ms[0]))
        # end to end, as a caller sees it: store.batch() with host indices (the sort, the prefix sum and two uploads included)
        t0 = time.perf_counter()
        b = store.batch(perm)
        torch.cuda.synchronize()
        emit(what="store.batch end to end", demos=n, frames=b.num_frames, seconds=time.perf_counter() - t0)
        del store, b, o_img, o_act, o_ep, o_done, o_mask, image

    if "epoch" in parts:
        class Model(torch.nn.Module):            # the shape of babyai/model.py's contract, small: what is timed is the loop around it
            memory_size = 128

            def __init__(self):
                super().__init__()
                self.emb = torch.nn.Embedding(40, 32)
                self.img = torch.nn.Linear(147, 64)
                self.rnn = torch.nn.GRUCell(64 + 32, 128)
                self.pi = torch.nn.Linear(128, 7)

            def _get_instr_embedding(self, instr):
                return self.emb(instr).sum(1)

            def forward(self, obs, memory, instr_embedding):
                x = torch.relu(self.img(obs.image.reshape(obs.image.shape[0], -1) / 16))
                memory = self.rnn(torch.cat([x, instr_embedding], dim=1), memory)
                return {"dist": torch.distributions.Categorical(logits=self.pi(memory)), "memory": memory}
        store = DemoStore.collect("BabyAI-GoToLocal-v0", 16384, 1000, batch=16384)
        model = Model().to(dev)
        opt = torch.optim.Adam(model.parameters(), 1e-4)
        perm = np.random.default_rng(1).permutation(len(store))
        imitation.run_epoch(model, store, perm[:1024], 256, 20, 0.01, optimizer=opt)        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = imitation.run_epoch(model, store, perm, 256, 20, 0.01, optimizer=opt)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        emit(what="run_epoch", level="BabyAI-GoToLocal-v0", demos=len(store), batch_size=256, recurrence=20, frames=log["total_frames"], seconds=dt,
             frames_per_s=log["total_frames"] / dt, note="host-bound: a small model, one process on a shared box")
    out.close()


if __name__ == "__main__":
    main()
