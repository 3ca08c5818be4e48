// bbai_grid.hpp -- the full-grid picture, MiniGridEnv.render('rgb_array', highlight, tile_size), as atlas tile ids: one id per
// cell of the W x H grid, from the live record's appearance plane, the pose and the highlight mask (k_render_grid; the host
// build of tests/test_grid_render_host.py checks it against the reference's frames).
//
// Reference semantics (gym_minigrid minigrid.py MiniGridEnv.render, restated in oracle/shim/gym_minigrid/minigrid.py:813-832;
// Grid.render :400-424): every cell is drawn as Grid.render_tile(cell, agent_dir if the agent stands there, highlight_mask[x, y]).
// highlight_mask = the cells of the 7x7 view that gen_obs_grid marks visible, projected to world coordinates (cells outside the
// grid dropped); the agent's own cell is always among them.  The carried object is not drawn.  The visibility comes out of the
// step's own view pipeline (bbai_view.hpp view_env_cells: an encoded view cell is visible iff its type is not 0).
//
// The fully observable encoding (full_cell, k_full_obs) is the same grid without pixels: FullyObsWrapper.observation (restated in
// oracle/shim/gym_minigrid/wrappers.py:39-56) = grid.encode() indexed [x][y], the agent's cell overwritten with (10 = agent, 0 = red, dir).
//
// Atlas lut (tools/gen_grid_atlas.py): lut[(highlight * 5 + agent) * 256 + key], agent = 0 or 1 + dir, key = appearance byte.
#pragma once
#include "bbai_types.hpp"
#include "bbai_view.hpp"

namespace bbai {

constexpr int GRID_LUT_BYTES = 2 * 5 * 256;

// hl[y] bit x = cell (x, y) is highlighted, y < c.H.
BB_HD void grid_highlight(const LevelCfg& c, const uint8_t* rec, const Hot& h, uint32_t* hl) {
    for (int y = 0; y < c.H; ++y) hl[y] = 0;
    uint32_t cp[13];
    (void)view_env_cells(c, rec, h, -1, cp);
    // DIR_TO_VEC: 0 (1, 0), 1 (0, 1), 2 (-1, 0), 3 (0, -1); right_vec = (-dy, dx)
    const int d = h.dir & 3;
    const int fx = d == 0 ? 1 : d == 2 ? -1 : 0, fy = d == 1 ? 1 : d == 3 ? -1 : 0;
    const int rx = -fy, ry = fx;
    const int tlx = h.ax + 6 * fx - 3 * rx, tly = h.ay + 6 * fy - 3 * ry;       // top_left = pos + f (V - 1) - r (V / 2)
    for (int vi = 0; vi < VIEW; ++vi)
        for (int vj = 0; vj < VIEW; ++vj) {
            const int k = VIEW * vi + vj;
            if (((cp[k >> 2] >> (8 * (k & 3))) & 7u) == 0) continue;
            const int x = tlx - fx * vj + rx * vi, y = tly - fy * vj + ry * vi;
            if ((unsigned)x < (unsigned)c.W && (unsigned)y < (unsigned)c.H) hl[y] |= 1u << x;
        }
    hl[h.ay] |= 1u << h.ax;
}

// The atlas tile of cell (x, y); highlight = 0: the reference's highlight=False (no cell highlighted).
// The two halves of that rule, each written once: which lut row the agent selects on cell (x, y), and the lut index.
BB_HD int grid_agent(const Hot& h, int x, int y) { return (x == h.ax && y == h.ay) ? 1 + (h.dir & 3) : 0; }
BB_HD int grid_lut_index(int lit, int agent, int key) { return (lit * 5 + agent) * 256 + key; }
BB_HD int grid_tile(const LevelCfg& c, const uint8_t* rec, const Hot& h, const uint8_t* lut, int highlight, const uint32_t* hl, int x, int y) {
    const int key = rec[e_index(c, x, y)];
    const int agent = grid_agent(h, x, y);
    const int lit = highlight ? (int)((hl[y] >> x) & 1u) : 0;
    return lut[grid_lut_index(lit, agent, key)];
}
// grid_tile_key: the same from the cell's appearance byte `key` with no cell highlighted (k_grid_delta reads the byte from rows staged in LDS).
BB_HD int grid_tile_key(int key, const Hot& h, const uint8_t* lut, int x, int y) { return lut[grid_lut_index(0, grid_agent(h, x, y), key)]; }

// All H x W tile ids of one env, row-major (ids[y * W + x]).
BB_HD void grid_tile_ids(const LevelCfg& c, const uint8_t* rec, const Hot& h, const uint8_t* lut, int highlight, uint8_t* ids) {
    uint32_t hl[MAX_W];
    grid_highlight(c, rec, h, hl);
    for (int y = 0; y < c.H; ++y)
        for (int x = 0; x < c.W; ++x) ids[y * c.W + x] = (uint8_t)grid_tile(c, rec, h, lut, highlight, hl, x, y);
}

// FullyObsWrapper's 3 bytes of cell (x, y): (type, colour, state) = the appearance byte's fields (engine.py grid_encoding), or
// (10, 0, dir) on the agent's cell.
constexpr int FULL_AGENT = 10;
// full_cell_key: the same from the cell's appearance byte `key` (k_full_obs reads it from rows staged in LDS).
BB_HD void full_cell_key(int key, const Hot& h, int x, int y, uint8_t* o) {
    const bool agent = x == h.ax && y == h.ay;
    o[0] = (uint8_t)(agent ? FULL_AGENT : key & 7);
    o[1] = (uint8_t)(agent ? 0 : (key >> 3) & 7);
    o[2] = (uint8_t)(agent ? (h.dir & 3) : key >> 6);
}
BB_HD void full_cell(const LevelCfg& c, const uint8_t* rec, const Hot& h, int x, int y, uint8_t* o) {
    full_cell_key(rec[e_index(c, x, y)], h, x, y, o);
}

// The whole frame of one env: out[(x * H + y) * 3 + k].
BB_HD void full_frame(const LevelCfg& c, const uint8_t* rec, const Hot& h, uint8_t* out) {
    for (int y = 0; y < c.H; ++y)
        for (int x = 0; x < c.W; ++x) full_cell(c, rec, h, x, y, out + (x * c.H + y) * 3);
}

}  // namespace bbai
