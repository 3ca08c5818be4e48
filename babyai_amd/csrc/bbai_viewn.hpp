// bbai_viewn.hpp -- the egocentric observation at any view size: gym-minigrid's ViewSizeWrapper(env, V) (RoomGridLevel passes
// agent_view_size through to MiniGridEnv, babyai/levels/levelgen.py:25-33; the expert reads mission.agent_view_size, babyai/bot.py:663-674).
// V is odd, 3 .. 11.  A frame is uint8[V][V][3], image[vi][vj][channel], the agent at view cell (V / 2, V - 1) facing up.
//
// Reference semantics (gen_obs_grid + Grid.encode, restated in oracle/shim/gym_minigrid/minigrid.py): a V x V window is cut at
// get_view_exts() -- a cell outside the grid is a wall --, rotated into the agent's frame, process_vis runs from the agent's cell, the
// agent's cell (always visible) shows the carried object, an unseen cell encodes as 0, 0, 0.  At V = 7 this is bbai_step.hpp observe_env.
//
// The start-carrying quirk (bonus_levels.py:821-829): on the PutNext...Carrying levels reset() builds its observation BEFORE it puts the
// object into the agent's hands, and ViewSizeWrapper does not observe again.  "The observation" is what the wrapped env last returned from
// reset() / step(): an env with hot.step == 0 and Prog.start_carry set shows the object on pos[start_carry] with app[start_carry] and the
// agent's cell empty -- what the 7x7 first observation of such an env shows (tests/test_full_obs_host.py::test_start_carrying_level_at_reset).
//
// Two forms of the same rule -- ONE body (observe_env_keys_n) over two ways of fetching a cell's appearance --, both compiled by the host
// tests (tests/test_view_size_host.py):
//   observe_env_n         the reference form: every cell read from the record's appearance plane;
//   observe_env_staged_n  the kernel's form on the host: the window staged as clamped dwords (view_win_dword), cells read from the stage
//                         (view_win_key) -- exactly the loads k_view_obs<V> issues, so the host build (and a sanitizer on it) checks the bounds.
// The appearance plane has MARGIN = 5 cells of wall around the grid; a 9x9 view reaches 8 cells ahead and an 11x11 view 10 ahead and 5 to
// the side: the window leaves the PLANE.  Every load is clamped to the plane and a cell outside [0, W) x [0, H) is a wall BY RULE -- a
// clamped load is never looked at (a cell inside the grid lies inside the plane, where nothing was clamped).
#pragma once
#include "bbai_types.hpp"
#include "bbai_step.hpp"

namespace bbai {

constexpr int VIEWN_MAX = 11;
BB_HD bool view_size_ok(int V) { return V >= 3 && V <= VIEWN_MAX && (V & 1); }
BB_HD int view_bytes(int V) { return 3 * V * V; }

// World cell shown at view cell (vi, vj): pos + f (V - 1 - vj) + r (vi - V / 2), r = (-f.y, f.x).  (view_to_world at V = 7)
BB_HD void view_to_world_n(int V, int ax, int ay, int dir, int vi, int vj, int& x, int& y) {
    const int fx = dir_dx(dir), fy = dir_dy(dir);
    const int rx = -fy, ry = fx;
    x = ax + fx * (V - 1 - vj) + rx * (vi - V / 2);
    y = ay + fy * (V - 1 - vj) + ry * (vi - V / 2);
}

// get_view_exts(): the window's top-left world cell.
BB_HD void view_top_left_n(int V, int ax, int ay, int dir, int& tx, int& ty) {
    const int d = dir & 3;
    tx = d == 0 ? ax : d == 2 ? ax - V + 1 : ax - V / 2;
    ty = d == 1 ? ay : d == 3 ? ay - V + 1 : ay - V / 2;
}

// Grid.process_vis on V-bit row masks.  opq[vj] bit vi = cell (vi, vj) blocks sight; returns vis[vj].  Agent at (V / 2, V - 1).
// (process_vis_rows at V = 7)
BB_HD void process_vis_rows_n(int V, const uint32_t* opq, uint32_t* vis) {
    const uint32_t all = (1u << V) - 1u, lo = all >> 1, hi = all & ~1u;
    uint32_t m = 1u << (V / 2);
    for (int vj = V - 1; vj >= 0; --vj) {
        const uint32_t t = ~opq[vj] & all;
        // left-to-right sweep (i = 0 .. V - 2): closure of  m[i + 1] |= m[i] & t[i]
        for (int k = 0; k < V - 1; ++k) m |= ((m & t & lo) << 1);
        const uint32_t a1 = m & t & lo;
        uint32_t up = a1 | (a1 << 1);
        // right-to-left sweep (i = V - 1 .. 1)
        for (int k = 0; k < V - 1; ++k) m |= ((m & t & hi) >> 1);
        const uint32_t a2 = m & t & hi;
        up |= a2 | (a2 >> 1);
        vis[vj] = m & all;
        m = up & all;
    }
}

// What the frame shows besides the plane: the agent's own cell, and the start-carrying quirk's object on its cell.
struct ViewExtra {
    int agent;          // appearance on the agent's cell: the carried object, or E_EMPTY
    int qx, qy, qapp;   // qx >= 0: world cell (qx, qy) shows qapp (the object reset() has not yet handed over)
};
BB_HD ViewExtra view_extra(const LevelCfg& c, const uint8_t* rec, const Hot& h) {
    ViewExtra x;
    x.agent = h.carry != NONE8 ? rec[c.off_app + h.carry] : (int)E_EMPTY;
    x.qx = x.qy = -1; x.qapp = E_EMPTY;
    const int sc = ((const Prog*)(rec + c.off_prog))->start_carry;
    if (h.step == 0 && sc != NONE8) {
        x.qx = rec[c.off_pos + 2 * sc]; x.qy = rec[c.off_pos + 2 * sc + 1]; x.qapp = rec[c.off_app + sc];
        x.agent = E_EMPTY;
    }
    return x;
}

// The override rule: what view cell (vi, vj), showing world cell (x, y) whose plane appearance is `key` (a wall outside the grid -- the
// caller's rule), shows.  Sight is decided on the PLANE's keys: neither object blocks it.  (Both host forms and k_view_obs's row stage.)
BB_HD int view_shown_n(int V, const ViewExtra& ex, int vi, int vj, int x, int y, int key) {
    if (x == ex.qx && y == ex.qy) key = ex.qapp;
    if (vi == V / 2 && vj == V - 1) key = ex.agent;
    return key;
}
// The three bytes of that cell.  (The agent's cell always comes out seen: process_vis_rows_n starts its sweep there.)
BB_HD void view_cell_n(int V, const ViewExtra& ex, int vi, int vj, int x, int y, int key, bool seen, uint8_t* o) {
    const int e = view_shown_n(V, ex, vi, vj, x, y, key);
    o[0] = (uint8_t)(seen ? e_type(e) : 0); o[1] = (uint8_t)(seen ? e_color(e) : 0); o[2] = (uint8_t)(seen ? e_state(e) : 0);
}

BB_HD bool in_grid(const LevelCfg& c, int x, int y) { return (unsigned)x < (unsigned)c.W && (unsigned)y < (unsigned)c.H; }

// gen_obs_grid + encode at view size V for one env, out[(vi * V + vj) * 3 + channel]; key_at(x, y) = the plane appearance of world cell (x, y).
template <class KeyAt>
BB_HD void observe_env_keys_n(const LevelCfg& c, const uint8_t* rec, const Hot& h, int V, KeyAt key_at, uint8_t* out) {
    uint32_t opq[VIEWN_MAX], vis[VIEWN_MAX];
    for (int vj = 0; vj < V; ++vj) {
        uint32_t o = 0;
        for (int vi = 0; vi < V; ++vi) {
            int x, y; view_to_world_n(V, h.ax, h.ay, h.dir, vi, vj, x, y);
            if (e_opaque(key_at(x, y))) o |= 1u << vi;
        }
        opq[vj] = o;
    }
    process_vis_rows_n(V, opq, vis);
    const ViewExtra ex = view_extra(c, rec, h);
    for (int vi = 0; vi < V; ++vi)
        for (int vj = 0; vj < V; ++vj) {
            int x, y; view_to_world_n(V, h.ax, h.ay, h.dir, vi, vj, x, y);
            view_cell_n(V, ex, vi, vj, x, y, key_at(x, y), (vis[vj] >> vi) & 1u, out + (vi * V + vj) * 3);
        }
}

// Reference form: every cell from the record's appearance plane.
BB_HD void observe_env_n(const LevelCfg& c, const uint8_t* rec, const Hot& h, int V, uint8_t* out) {
    observe_env_keys_n(c, rec, h, V, [&](int x, int y) { return in_grid(c, x, y) ? rec[e_index(c, x, y)] : (int)E_WALL; }, out);
}

// ---- the staged window: V rows of ND dwords, what k_view_obs<V> loads ------------------------------------------------------------
// Row r of the stage = plane row ty + MARGIN + r (clamped to [0, EH)), dwords d0 .. d0 + ND - 1 of it (each clamped to [0, ES / 4)),
// d0 = floor((tx + MARGIN) / 4): window column i is byte ph + i of the row, ph = (tx + MARGIN) - 4 d0 in 0 .. 3.  ES is a multiple of 4 and
// records are 64-byte aligned, so the dwords are aligned.
BB_HD constexpr int view_nd(int V) { return (V + 6) / 4; }        // 2, 2, 3, 3, 4
BB_HD int view_win_d0(int tx) { return (tx + MARGIN + 16) / 4 - 4; }              // (tx + MARGIN >= -16: a floor, not a truncation)
// index into the record's dwords
BB_HD int view_win_dword(const LevelCfg& c, int tx, int ty, int r, int k) {
    int py = ty + MARGIN + r, d = view_win_d0(tx) + k;
    py = py < 0 ? 0 : py >= c.EH ? c.EH - 1 : py;
    d = d < 0 ? 0 : d >= c.ES / 4 ? c.ES / 4 - 1 : d;
    return py * (c.ES / 4) + d;
}
// the appearance of world cell (x, y) of the window, `row` = the ND staged dwords of its row as bytes
BB_HD int view_win_key(const LevelCfg& c, int tx, int x, int y, const uint8_t* row) {
    return in_grid(c, x, y) ? row[(tx + MARGIN - 4 * view_win_d0(tx)) + (x - tx)] : (int)E_WALL;
}

// The kernel's form on the host: stage, then cells from the stage.
BB_HD void observe_env_staged_n(const LevelCfg& c, const uint8_t* rec, const Hot& h, int V, uint8_t* out) {
    const int ND = view_nd(V);
    uint32_t win[VIEWN_MAX * 4];
    int tx, ty; view_top_left_n(V, h.ax, h.ay, h.dir, tx, ty);
    for (int r = 0; r < V; ++r)
        for (int k = 0; k < ND; ++k) win[r * ND + k] = ((const uint32_t*)rec)[view_win_dword(c, tx, ty, r, k)];
    observe_env_keys_n(c, rec, h, V, [&](int x, int y) { return view_win_key(c, tx, x, y, (const uint8_t*)(win + (y - ty) * ND)); }, out);
}

}  // namespace bbai

#if defined(__HIPCC__)
#include "bbai_kernels.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_view_obs<V> : ViewSizeWrapper(env, V).observation of listed envs (bbai_observe_view, bbai_step_view)
// ------------------------------------------------------------------------------------------
// Work item = ViewN<V>::EPI envs (a multiple of 16: F = 3 V^2 is odd, so every item's range of `out` starts 16-byte aligned and only the
// end of the whole output can hold a partial chunk, stored byte by byte).  Per item a block
//   1. (one lane per env) has the env's id and Hot in registers -- loaded under the previous item's work --, finds the live record
//      and parks both in LDS (the item skeleton k_full_obs is built from as well: bbai_kernels.hpp, list_item_load / _park);
//   2. issues ALL loads of the item before the first use: the V x ND clamped dwords of every env's window (view_win_dword; ITER independent
//      loads per lane, statically indexed registers), and per env the carried object's appearance and Prog.start_carry -- ONE round trip.
//      Only an env of a start-carrying level at step 0 pays a second one (its object's cell and appearance);
//   3. a lane per view row vj: the row's V appearance bytes (view_win_key; the agent's cell and the quirk's cell as view_shown_n overrides
//      them) parked in LDS in output order [vi][vj], and its opacity mask; then process_vis_rows_n, a lane per env, in place; then the
//      cells, FOUR per lane: one dword of parked keys in, the visibility bits, twelve bytes = three dwords into the item's frames in LDS
//      at the output pitch (cell k of the item is bytes 3 k .. 3 k + 2 of its frames);
//   4. stores the frames -- ONE contiguous byte range of `out` -- as 16-byte nontemporal chunks (list_item_store).
// Writes nothing but `out`; an id outside [0, n) gives an all-zero frame.  No scratch: every register array is indexed statically.
constexpr int VIEWN_BLOCK = 256;
constexpr int VIEWN_BPC = 4;                  // persistent blocks per CU

template <int V> struct ViewN {
    static constexpr int F = 3 * V * V;                           // 27, 75, 147, 243, 363
    static constexpr int ND = view_nd(V);
    static constexpr int EPI = V == 3 ? 256 : V == 5 ? 128 : V == 7 ? 96 : V == 9 ? 64 : 48;      // envs per work item: 6.9, 9.6, 14.1, 15.6, 17.4 KB
                                                                  // of frames; with the stage, the keys and the per-env rows 29, 26, 33, 33, 36 KB of LDS: four blocks per CU
    static constexpr int WIN = V * ND;                            // staged dwords per env
    static constexpr int ITER = (EPI * WIN + VIEWN_BLOCK - 1) / VIEWN_BLOCK;
    static_assert(EPI % 16 == 0 && EPI <= VIEWN_BLOCK, "item shape");
};

struct ViewNArgs {
    EnvList list;                // the batch, the listed envs, their frames (bbai_kernels.hpp)
    int64_t items;
};
static_assert(sizeof(ViewNArgs) == 264 && offsetof(ViewNArgs, items) == 256, "k_view_obs's argument layout");

template <int V>
__global__ __launch_bounds__(VIEWN_BLOCK, 4) void k_view_obs(ViewNArgs a) {
    using G = ViewN<V>;
    constexpr int EPI = G::EPI, F = G::F, ND = G::ND, WIN = G::WIN, ITER = G::ITER;
    __shared__ __attribute__((aligned(16))) uint8_t s_frames[EPI * F];
    __shared__ __attribute__((aligned(16))) uint32_t s_win[EPI * WIN];
    __shared__ __attribute__((aligned(16))) Hot s_hot[EPI];
    __shared__ const uint8_t* s_rec[EPI];
    __shared__ ViewExtra s_ex[EPI];
    __shared__ uint32_t s_row[EPI * V];           // opacity rows, then visibility rows
    __shared__ __attribute__((aligned(16))) uint8_t s_key[EPI * V * V];      // the cells' appearance bytes, [env][vi][vj]
    const int tid = threadIdx.x;
    const EnvList& l = a.list;
    u32x4 h = {0u, 0u, 0u, 0u};
    int64_t item = blockIdx.x;
    int64_t env = item < a.items ? list_item_load(l, item, EPI, tid, h) : -1;
    for (; item < a.items; item += gridDim.x) {
        const int64_t first = item * EPI;
        const int ne = list_item_envs(l, first, EPI);
        __syncthreads();                                  // the previous item's frames are stored
        if (tid < ne) list_item_park(l, tid, env, h, s_hot, s_rec);
        __syncthreads();
        {   // every load of the item, then its uses
            uint32_t v[ITER];
            int ce = E_EMPTY, sc = NONE8;
            const uint8_t* myrec = tid < ne ? s_rec[tid] : nullptr;
            const Hot myhot = s_hot[tid < ne ? tid : 0];
#pragma unroll
            for (int u = 0; u < ITER; ++u) {
                const int k = tid + u * VIEWN_BLOCK;
                v[u] = 0;
                if (k < ne * WIN) {
                    const int e = k / WIN, w = k - e * WIN, r = w / ND, d = w - r * ND;
                    const uint8_t* rec = s_rec[e];
                    if (rec) {
                        const Hot hh = s_hot[e];
                        int tx, ty; view_top_left_n(V, hh.ax, hh.ay, hh.dir, tx, ty);
                        v[u] = ((const uint32_t*)rec)[view_win_dword(l.c, tx, ty, r, d)];
                    }
                }
            }
            if (myrec) {
                if (myhot.carry != NONE8 && myhot.carry < l.c.maxo) ce = myrec[l.c.off_app + myhot.carry];
                sc = myrec[l.c.off_prog + (int)offsetof(Prog, start_carry)];
            }
#pragma unroll
            for (int u = 0; u < ITER; ++u)
                if (tid + u * VIEWN_BLOCK < ne * WIN) s_win[tid + u * VIEWN_BLOCK] = v[u];
            if (tid < ne) {
                ViewExtra ex;
                ex.agent = ce; ex.qx = ex.qy = -1; ex.qapp = E_EMPTY;
                if (myrec && myhot.step == 0 && sc != NONE8 && sc < l.c.maxo) {      // the start-carrying quirk: a second round trip, at reset only
                    ex.qx = myrec[l.c.off_pos + 2 * sc]; ex.qy = myrec[l.c.off_pos + 2 * sc + 1]; ex.qapp = myrec[l.c.off_app + sc];
                    ex.agent = E_EMPTY;
                }
                s_ex[tid] = ex;
            }
        }
        env = item + gridDim.x < a.items ? list_item_load(l, item + gridDim.x, EPI, tid, h) : -1;      // the next item's entries, under this item's work
        __syncthreads();
        for (int k = tid; k < ne * V; k += VIEWN_BLOCK) {             // view row vj of env e: its keys and its opacity mask
            const int e = k / V, vj = k - e * V;
            uint32_t o = 0;
            uint8_t* keys = s_key + e * (V * V) + vj;
            if (s_rec[e]) {
                const Hot hh = s_hot[e];
                const ViewExtra ex = s_ex[e];
                int tx, ty; view_top_left_n(V, hh.ax, hh.ay, hh.dir, tx, ty);
#pragma unroll
                for (int vi = 0; vi < V; ++vi) {
                    int x, y; view_to_world_n(V, hh.ax, hh.ay, hh.dir, vi, vj, x, y);
                    int key = view_win_key(l.c, tx, x, y, (const uint8_t*)(s_win + e * WIN + (y - ty) * ND));
                    if (e_opaque(key)) o |= 1u << vi;
                    keys[vi * V] = (uint8_t)view_shown_n(V, ex, vi, vj, x, y, key);
                }
            } else {
#pragma unroll
                for (int vi = 0; vi < V; ++vi) keys[vi * V] = 0;                    // an id outside [0, n): every cell encodes as 0, 0, 0
            }
            s_row[k] = o;
        }
        __syncthreads();
        if (tid < ne) process_vis_rows_n(V, s_row + tid * V, s_row + tid * V);      // in place (row vj is read before it is written); pitch V is odd: no bank
                                                                                    // conflict.  The agent's cell comes out visible: the sweep starts there
        __syncthreads();
        for (int k = 4 * tid; k < ne * (V * V); k += 4 * VIEWN_BLOCK) {             // cells k .. k + 3 (past the item's last env: unused bytes of the arrays)
            const uint32_t keys = *(const uint32_t*)(s_key + k);
            int e = k / (V * V), w = k - e * (V * V), vi = w / V, vj = w - vi * V;
            uint32_t b[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t key = (keys >> (8 * c)) & 0xFFu;
                const uint32_t seen = e < ne ? (s_row[e * V + vj] >> vi) & 1u : 0u;
                b[c] = seen ? (key & 7u) | (((key >> 3) & 7u) << 8) | ((key >> 6) << 16) : 0u;      // (type, colour, state)
                if (++vj == V) { vj = 0; if (++vi == V) { vi = 0; ++e; } }
            }
            uint32_t* o = (uint32_t*)(s_frames + 3 * k);                            // (k is a multiple of 4: 12-byte steps from a 16-byte base)
            o[0] = b[0] | (b[1] << 24);
            o[1] = (b[1] >> 8) | (b[2] << 16);
            o[2] = (b[2] >> 16) | (b[3] << 8);
        }
        __syncthreads();
        list_item_store<VIEWN_BLOCK>(l.out + first * F, s_frames, ne * F, tid);      // 16-byte aligned (see above)
    }
}
#endif
