// bbai_dirty.hpp -- the arithmetic of step_dirty (bbai_stepk.hpp), four cells per word: the tile ids of a 16-cell shadow chunk from its 48
// encoding bytes, and the chunk's changed cells as 16 bits.  Plain C++ (bb_perm is v_perm_b32 on the device and a portable twin on the
// host), so that the host tests run the very functions the kernel runs: tests/test_step_dirty_host.py holds each of them against the
// per-cell definition (tile_id of bbai_render.hpp, a compare per id) for every first cell, every live count and the extreme encodings.
#pragma once
#include "bbai_types.hpp"
#include "bbai_view.hpp"

namespace bbai {

constexpr int DIRTY_CELLS = VIEW * VIEW;              // cells per env: a chunk's first cell is (16 x chunk) mod 49
constexpr int DIRTY_AGENT = 3 * VIEW + 6;             // the agent's own cell (AGENT_CELL of bbai_kernels.hpp; step_dirty asserts the two equal)
constexpr int DIRTY_CHUNK = 16;                       // cells per chunk = shadow bytes per 16-byte load

// The lut keys of four cells at once.  Their 12 encoding bytes are three dwords, a = t0 c0 s0 t1, b = c1 s1 t2 c2, c = s2 t3 c3 s3 from the
// low byte up: six byte permutes gather the types, the colours and the states into a word each, and key = type | colour << 3 | state << 6
// (tile_id) is formed on the whole words.
// BOUND: a shifted byte must not spill into its neighbour -- colour < 32 and state < 4 in every byte.  encode_cells_to / encode_view emit
// type = e & 7, colour = (e >> 3) & 7, state = e >> 6 of an appearance byte e, so colour <= 7 and state <= 3 for every encoding the step
// can write, and a frozen or held env re-emits bytes an earlier step wrote; tools/gen_atlas.py builds the lut for these keys (256 entries
// per table: type | colour << 3 | state << 6 <= 255).  A byte past the bound would change the neighbouring cell's key here, where the
// per-cell form read past the table instead.
BB_HD uint32_t dirty_keys4(uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t t = bb_perm(c, bb_perm(b, a, 0x0C060300u), 0x05020100u);      // a0 a3 b2 c1
    const uint32_t col = bb_perm(c, bb_perm(b, a, 0x0C070401u), 0x06020100u);    // a1 b0 b3 c2
    const uint32_t st = bb_perm(c, bb_perm(b, a, 0x0C0C0502u), 0x07040100u);     // a2 b1 c0 c3
    return t | (col << 3) | (st << 6);
}

// Four tile ids from four keys (a byte each), packed like the shadow: the plain table, lut[0 .. 255].
BB_HD uint32_t dirty_ids4(const uint8_t* lut, uint32_t keys) {
    return (uint32_t)lut[keys & 0xFFu] | (uint32_t)lut[(keys >> 8) & 0xFFu] << 8 | (uint32_t)lut[(keys >> 16) & 0xFFu] << 16 | (uint32_t)lut[keys >> 24] << 24;
}

// Where the agent's cell lies in the chunk whose first cell is `c0` (0 .. 48): its index 0 .. 15, or -1.  A chunk is 16 cells and an env 49:
// no chunk holds two.
BB_HD int dirty_agent_index(int c0) {
    int i = DIRTY_AGENT - c0;
    if (i < 0) i += DIRTY_CELLS;
    return i < DIRTY_CHUNK ? i : -1;
}

// "byte != 0" of a word's four bytes as four adjacent bits (bit j = byte j).  The masked add carries into bit 7 of a byte iff one of its low
// seven bits is set and never out of the byte; the multiply then moves the flags of bytes 0, 1, 2, 3 (bits 0, 8, 16, 24) to bits 21, 22,
// 23, 24 -- the sixteen partial products fall on distinct bits (0 7 14 21 | 8 15 22 29 | 16 23 30 | 24 31; the rest past bit 31), so none carries.
BB_HD uint32_t dirty_flags4(uint32_t x) {
    const uint32_t f = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    return (((f >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// A chunk's 16 dirty bits (bit i = cell c0 + i) split at the env boundary: `ma` = the bits of the chunk's first env at their cells, `mb` =
// those of the next env.  c0 <= 48 and 16 bits: the shifted word ends at bit 63.
BB_HD void dirty_split(uint32_t bits, int c0, uint64_t& ma, uint64_t& mb) {
    const uint64_t m = (uint64_t)bits << c0;
    ma = m & ((1ull << DIRTY_CELLS) - 1ull);
    mb = m >> DIRTY_CELLS;
}

// One chunk: `ew` = its 48 encoding bytes, `old` = its 16 shadow bytes, c0 = its first cell, `live` = how many of its cells exist (>= 16
// but in the last chunk of a partial block; bytes of `old` past them are ignored).  Writes the new ids to `nw` (bytes past `live`: unspecified) and returns the
// changed cells among the live ones, bit i = cell i of the chunk.  `lut` = the plain table and, 256 bytes on, the agent's.
BB_HD uint32_t dirty_chunk(const uint32_t* ew, const uint32_t* old, const uint8_t* lut, int c0, int live, uint32_t* nw) {
    uint32_t keys[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        keys[g] = dirty_keys4(ew[3 * g], ew[3 * g + 1], ew[3 * g + 2]);
        nw[g] = dirty_ids4(lut, keys[g]);
    }
    const int ia = dirty_agent_index(c0);
    if (ia >= 0) {                                    // the one id of the agent's table (selects, not indexed registers)
        const int sh = 8 * (ia & 3);
        uint32_t kw = keys[0];
#pragma unroll
        for (int g = 1; g < 4; ++g) kw = (ia >> 2) == g ? keys[g] : kw;
        const uint32_t id = lut[256 + ((kw >> sh) & 0xFFu)];
#pragma unroll
        for (int g = 0; g < 4; ++g) nw[g] = (ia >> 2) == g ? (nw[g] & ~(0xFFu << sh)) | id << sh : nw[g];
    }
    uint32_t bits = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) bits |= dirty_flags4(nw[g] ^ old[g]) << (4 * g);
    return live >= DIRTY_CHUNK ? bits : bits & ((1u << live) - 1u);
}

}  // namespace bbai
