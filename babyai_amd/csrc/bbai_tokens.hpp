// bbai_tokens.hpp -- the small kernels around a training loop's step.
//   k_tokens       lane = env: mission text as fixed-vocabulary token ids of the envs that started a new episode.
//   k_tap          the outputs of listed envs into log rows (bbai_tap_ids; bench.py's parity tap).
//   k_gae          generalised advantage estimation of a rollout, lane = env.
// Part of bbai_engine.hip's translation unit: included where the code stood, at global scope.  The launches are bbai_engine.hip's
// (window_end, tap_launch, bbai_gae).
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_tokens : mission strings as fixed-vocabulary token ids, produced on the device from the compiled
// instruction program (grammar: babyai/levels/verifier.py:64-94,248-249,287-288,318-319,366-367,439-440,
// 480-481,526-527).  Vocabulary ids = babyai_amd/missions.py VOCAB (1..32, 0 = padding).
// ------------------------------------------------------------------------------------------
constexpr int TOK_MAX = 72;      // longest sentence: two And-pairs of put-next clauses with locations
struct TokOut {
    uint8_t* p; int n;
    __device__ __forceinline__ void put(int id) { if (n < TOK_MAX) p[n++] = (uint8_t)id; }
};
__device__ __forceinline__ void tok_desc(TokOut& o, DescInfo d) {
    o.put(d.count > 1 ? 9 : 8);                         // a / the
    if (d.color != 7) o.put(11 + d.color);              // red green blue purple yellow grey
    o.put(d.type == 0 ? 10 : 24 - d.type);              // object | box ball key door
    if (d.loc == LOC_FRONT) { o.put(21); o.put(22); o.put(23); o.put(24); }      // in front of you
    else if (d.loc == LOC_BEHIND) { o.put(25); o.put(24); }                     // behind you
    else if (d.loc == LOC_LEFT) { o.put(26); o.put(27); o.put(28); }            // on your left
    else if (d.loc == LOC_RIGHT) { o.put(26); o.put(27); o.put(29); }           // on your right
}
__device__ __forceinline__ void tok_side(TokOut& o, const Prog* p, int base, int n) {
    for (int q = 0; q < n; ++q) {
        if (q) o.put(30);                                                        // and
        const int kind = p->kind[base + q];
        if (kind == L_GOTO) { o.put(1); o.put(2); }                              // go to
        else if (kind == L_PICKUP) { o.put(3); o.put(4); }                       // pick up
        else if (kind == L_OPEN) o.put(5);                                       // open
        else o.put(6);                                                           // put
        tok_desc(o, p->desc[base + q][0]);
        if (kind == L_PUTNEXT) { o.put(7); o.put(2); tok_desc(o, p->desc[base + q][1]); }   // next to
    }
}
__global__ __launch_bounds__(64) void k_tokens(LevelCfg c, int64_t n, const uint8_t* __restrict__ recs, const uint8_t* __restrict__ ring /* in-place layout, else NULL */, int depth,
                                               const Hot* __restrict__ hots, uint8_t* __restrict__ tokens,
                                               const int32_t* __restrict__ reset_list, const uint32_t* __restrict__ counter,
                                               int mode /* 0: the reset list (unfused consume); 1: every env; 2: the envs whose `dones` byte is set -- a fused / in-place
                                                           auto-reset step keeps no list, and there done == "a new episode started" */,
                                               const uint8_t* __restrict__ dones) {
    const int64_t count = mode ? n : (int64_t)counter[0];
    for (int64_t it = (int64_t)blockIdx.x * 64 + threadIdx.x; it < count; it += (int64_t)gridDim.x * 64) {
        const int64_t env = mode ? it : (int64_t)reset_list[it];
        if (mode == 2 && !dones[env]) continue;
        const Prog* p = (const Prog*)(live_rec(c, n, env, (uint8_t*)recs, (uint8_t*)ring, depth, ring ? hots[env].slot : 0) + c.off_prog);
        TokOut o; o.p = tokens + env * TOK_MAX; o.n = 0;
        tok_side(o, p, 0, p->n_a);
        if (p->root == R_BEFORE) { o.put(31); tok_side(o, p, 2, p->n_b); }                   // , then
        else if (p->root == R_AFTER) { o.put(32); o.put(24); tok_side(o, p, 2, p->n_b); }    // after you
        while (o.n < TOK_MAX) o.p[o.n++] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// k_tap : copy the outputs of `count` envs (and the pixels of the first `pix_count` of them) into log rows -- the parity
// tap of bench.py as ONE launch inside the timed region (five small tensor copies cost more than a 65 536-env step).
// ids == NULL: the first `count` envs; else env ids[k] -> log row k (any order, anywhere in the batch).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tap(int64_t count, int64_t pix_count, const int64_t* __restrict__ ids, const uint8_t* __restrict__ image,
                                             const uint8_t* __restrict__ dirs, const double* __restrict__ rew64, const uint8_t* __restrict__ dones,
                                             const uint8_t* __restrict__ pixels, uint8_t* __restrict__ image_out, uint8_t* __restrict__ dirs_out,
                                             double* __restrict__ rew64_out, uint8_t* __restrict__ dones_out, uint8_t* __restrict__ pixels_out) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < count * OBS_BYTES; i += nth) {
        const int64_t k = i / OBS_BYTES, b = i - k * OBS_BYTES;
        image_out[i] = image[(ids ? ids[k] : k) * OBS_BYTES + b];
    }
    for (int64_t i = tid; i < count; i += nth) {
        const int64_t e = ids ? ids[i] : i;
        dirs_out[i] = dirs[e]; dones_out[i] = dones[e]; rew64_out[i] = rew64[e];
    }
    constexpr int VEC = PIX_BYTES / 16;
    const u32x4* src = (const u32x4*)pixels;
    u32x4* dst = (u32x4*)pixels_out;
    for (int64_t i = tid; i < pix_count * VEC; i += nth) {
        const int64_t k = i / VEC, v = i - k * VEC;
        dst[i] = src[(ids ? ids[k] : k) * VEC + v];
    }
}

// ------------------------------------------------------------------------------------------
// k_gae : generalised advantage estimation of a rollout, lane = env (babyai/rl/algos/base.py:196-202 as ONE reverse
// scan per env instead of T passes of five tensor ops).  All buffers are env-major [P][T], the layout the reference
// flattens its experiences to (base.py:207-232), so nothing is transposed afterwards.  float32 arithmetic in the
// reference's operation order (python scalars multiply as float32; the file is built with -ffp-contract=off):
//   delta = (r + (d * next_value) * next_mask) - v ;  adv = delta + ((d * lambda) * next_adv) * next_mask
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_gae(int64_t P, int T, const float* __restrict__ rewards, const float* __restrict__ values,
                                            const float* __restrict__ masks, const float* __restrict__ last_mask,
                                            const float* __restrict__ last_value, float d, float dl, float* __restrict__ adv,
                                            float* __restrict__ ret) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const float* r = rewards + p * T; const float* v = values + p * T; const float* m = masks + p * T;
    float next_value = last_value[p], next_mask = last_mask[p], next_adv = 0.0f;
    for (int i = T - 1; i >= 0; --i) {
        const float vi = v[i];
        const float delta = (r[i] + (d * next_value) * next_mask) - vi;
        const float a = delta + (dl * next_adv) * next_mask;
        adv[p * T + i] = a;
        ret[p * T + i] = vi + a;
        next_value = vi; next_mask = m[i]; next_adv = a;
    }
}
