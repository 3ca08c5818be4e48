// The word-parallel arithmetic of step_dirty (babyai_amd/csrc/bbai_dirty.hpp) against the per-cell definition, written out plainly here:
// tile_id per cell (key = type | colour << 3 | state << 6, the agent's table at cell 27), a bit per differing id among the live cells, the
// bits split at the env boundary.  A stand-alone program: tests/test_step_dirty_host.py compiles it plain and with the address and
// undefined-behaviour sanitizers and runs both.  Exit status 0 and a last line "ok ..." = every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bbai_dirty.hpp"

using namespace bbai;

static long checks = 0, failures = 0;
static void fail(const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
    if (++failures <= 20) std::printf("FAIL %s (%ld, %ld, %ld, %ld)\n", what, a, b, c, d);
}
#define CHECK(cond, ...) do { ++checks; if (!(cond)) fail(__VA_ARGS__); } while (0)

// xorshift64*: the same stream in both builds
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

constexpr int CELLS_ = 49, AGENT_ = 27;

// ---- the per-cell definition ------------------------------------------------------------------------------------------------------
static uint8_t ref_tile_id(const uint8_t* lut, int o0, int o1, int o2, int cell) {
    const int key = o0 | (o1 << 3) | (o2 << 6);
    return lut[(cell == AGENT_ ? 256 : 0) + key];
}
struct RefChunk { uint8_t id[16]; uint32_t bits; uint64_t ma, mb; };
static RefChunk ref_chunk(const uint8_t* enc /* 48 */, const uint8_t* old /* 16 */, const uint8_t* lut, int c0, int live) {
    RefChunk r;
    std::memset(&r, 0, sizeof r);
    int cell = c0;
    bool second = false;
    for (int i = 0; i < 16; ++i) {
        if (i < live) {
            r.id[i] = ref_tile_id(lut, enc[3 * i], enc[3 * i + 1], enc[3 * i + 2], cell);
            if (r.id[i] != old[i]) {
                r.bits |= 1u << i;
                if (second) r.mb |= 1ull << cell; else r.ma |= 1ull << cell;
            }
        }
        if (++cell == CELLS_) { cell = 0; second = true; }
    }
    return r;
}

// ---- the code under test, on bytes ------------------------------------------------------------------------------------------------
static uint32_t word_at(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static void check_chunk(const uint8_t* enc, const uint8_t* old, const uint8_t* lut, int c0, int live, int tag) {
    uint32_t ew[12], ow[4], nw[4] = {0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu};
    for (int j = 0; j < 12; ++j) ew[j] = word_at(enc + 4 * j);
    for (int j = 0; j < 4; ++j) ow[j] = word_at(old + 4 * j);
    const uint32_t bits = dirty_chunk(ew, ow, lut, c0, live, nw);
    uint64_t ma = ~0ull, mb = ~0ull;
    dirty_split(bits, c0, ma, mb);
    const RefChunk r = ref_chunk(enc, old, lut, c0, live);
    CHECK(bits == r.bits, "dirty bits", tag, c0, live, (long)(bits ^ r.bits));
    CHECK(ma == r.ma && mb == r.mb, "split at the env boundary", tag, c0, live, (long)bits);
    for (int i = 0; i < live; ++i) CHECK(((nw[i >> 2] >> (8 * (i & 3))) & 0xFFu) == r.id[i], "tile id", tag, c0, live, i);
}

// An encoding byte triple from the reachable ranges (type 0..7, colour 0..7, state 0..3: what encode_cells_to can emit), the extreme
// values of each more often than a uniform draw would give them.
static void draw_cell(uint8_t* e) {
    const uint32_t r = rnd();
    e[0] = (uint8_t)((r & 3) == 0 ? ((r >> 2 & 1) ? 7 : 0) : (r >> 8) & 7);
    e[1] = (uint8_t)((r >> 3 & 3) == 0 ? ((r >> 5 & 1) ? 7 : 0) : (r >> 12) & 7);
    e[2] = (uint8_t)((r >> 6 & 3) == 0 ? ((r >> 16 & 1) ? 3 : 0) : (r >> 20) & 3);
}

enum { LUT_RANDOM = 0, LUT_AGENT_DIFFERS = 1, LUT_SHARED = 2, LUT_KINDS = 3 };
static void make_lut(int kind, uint8_t* lut) {
    for (int k = 0; k < 256; ++k) {
        if (kind == LUT_RANDOM) { lut[k] = (uint8_t)rnd(); lut[256 + k] = (uint8_t)rnd(); }
        else if (kind == LUT_AGENT_DIFFERS) { lut[k] = (uint8_t)rnd(); lut[256 + k] = (uint8_t)(lut[k] ^ (1 + rnd() % 255)); }      // the agent's id differs on EVERY key
        else { lut[k] = (uint8_t)(k % 3); lut[256 + k] = (uint8_t)(3 + k % 2); }                                                     // many keys share an id
    }
}

static void test_flags() {
    // all 16 zero / non-zero patterns, every non-zero byte at each of the values whose bits sit at the ends of the masked add
    static const uint8_t nz[] = {0x01, 0x7F, 0x80, 0xFF, 0x02, 0x40, 0x81, 0xFE};
    for (int pat = 0; pat < 16; ++pat)
        for (int v0 = 0; v0 < 8; ++v0) for (int v1 = 0; v1 < 8; ++v1) for (int v2 = 0; v2 < 8; ++v2) for (int v3 = 0; v3 < 8; ++v3) {
            const uint32_t x = (pat & 1 ? nz[v0] : 0u) | (pat & 2 ? nz[v1] : 0u) << 8 | (pat & 4 ? nz[v2] : 0u) << 16 | (pat & 8 ? (uint32_t)nz[v3] : 0u) << 24;
            CHECK(dirty_flags4(x) == (uint32_t)pat, "byte flags", pat, (long)x);
        }
    // every value of one byte, the other three all zero or all 0xFF
    for (int j = 0; j < 4; ++j) for (int v = 0; v < 256; ++v) {
        const uint32_t lo = (uint32_t)v << (8 * j), hi = lo | (0xFFFFFFFFu & ~(0xFFu << (8 * j)));
        CHECK(dirty_flags4(lo) == (v ? 1u << j : 0u), "byte flags, one byte", j, v);
        CHECK(dirty_flags4(hi) == ((v ? 1u << j : 0u) | (0xFu & ~(1u << j))), "byte flags, one byte among 0xFF", j, v);
    }
    for (int k = 0; k < 200000; ++k) {
        uint32_t x = rnd();
        const uint32_t z = rnd();
        for (int j = 0; j < 4; ++j) if (z >> j & 1) x &= ~(0xFFu << (8 * j));
        uint32_t want = 0;
        for (int j = 0; j < 4; ++j) want |= ((x >> (8 * j)) & 0xFFu ? 1u : 0u) << j;
        CHECK(dirty_flags4(x) == want, "byte flags, random", (long)x);
    }
}

static void test_keys() {
    // every reachable (type, colour, state) in every one of the four positions, the other three cells drawn
    for (int pos = 0; pos < 4; ++pos) for (int t = 0; t < 8; ++t) for (int c = 0; c < 8; ++c) for (int s = 0; s < 4; ++s) {
        uint8_t e[12];
        for (int i = 0; i < 4; ++i) draw_cell(e + 3 * i);
        e[3 * pos] = (uint8_t)t; e[3 * pos + 1] = (uint8_t)c; e[3 * pos + 2] = (uint8_t)s;
        const uint32_t k = dirty_keys4(word_at(e), word_at(e + 4), word_at(e + 8));
        for (int i = 0; i < 4; ++i)
            CHECK(((k >> (8 * i)) & 0xFFu) == (uint32_t)(e[3 * i] | (e[3 * i + 1] << 3) | (e[3 * i + 2] << 6)), "key", pos, i, t | c << 3 | s << 6);
    }
    // the bound the word-wide shifts rely on, at its edge: colour 31 and state 3 in every cell still give each cell its own key
    uint8_t e[12];
    for (int i = 0; i < 4; ++i) { e[3 * i] = 0xFF; e[3 * i + 1] = 31; e[3 * i + 2] = 3; }
    CHECK(dirty_keys4(word_at(e), word_at(e + 4), word_at(e + 8)) == 0xFFFFFFFFu, "key at the bound");
    for (int i = 0; i < 4; ++i) { e[3 * i] = 0; e[3 * i + 1] = (uint8_t)(i & 1 ? 31 : 0); e[3 * i + 2] = (uint8_t)(i & 1 ? 0 : 3); }
    CHECK(dirty_keys4(word_at(e), word_at(e + 4), word_at(e + 8)) == 0xF8C0F8C0u, "neighbouring keys at the bound");
}

static void test_agent_and_split() {
    for (int c0 = 0; c0 < CELLS_; ++c0) {
        int want = -1, found = 0;
        for (int i = 0; i < 16; ++i) if ((c0 + i) % CELLS_ == AGENT_) { want = i; ++found; }
        CHECK(found <= 1 && dirty_agent_index(c0) == want, "agent's index in the chunk", c0, want);
        for (int rep = 0; rep < 40; ++rep) {
            const uint32_t bits = rep < 16 ? 1u << rep : rep == 16 ? 0u : rep == 17 ? 0xFFFFu : rnd() & 0xFFFFu;
            uint64_t ma = 0, mb = 0, ra = 0, rb = 0;
            for (int i = 0; i < 16; ++i) if (bits >> i & 1) { if (c0 + i < CELLS_) ra |= 1ull << (c0 + i); else rb |= 1ull << (c0 + i - CELLS_); }
            dirty_split(bits, c0, ma, mb);
            CHECK(ma == ra && mb == rb, "split", c0, (long)bits);
        }
    }
}

static void test_chunks() {
    static const uint8_t flips[] = {0x01, 0x7F, 0x80, 0xFF};
    uint8_t lut[512], enc[48], enc2[48], old[16];
    for (int kind = 0; kind < LUT_KINDS; ++kind) for (int rep = 0; rep < 3; ++rep) {
        make_lut(kind, lut);
        for (int c0 = 0; c0 < CELLS_; ++c0) for (int live = 1; live <= 16; ++live) {
            for (int i = 0; i < 16; ++i) draw_cell(enc + 3 * i);
            if (rep == 1) std::memset(enc, 0, sizeof enc);                                   // the extreme encodings in every cell at once
            if (rep == 2) for (int i = 0; i < 16; ++i) { enc[3 * i] = 7; enc[3 * i + 1] = 7; enc[3 * i + 2] = 3; }
            const RefChunk same = ref_chunk(enc, enc /* unused: ids only */, lut, c0, 16);
            // old ids equal: nothing is dirty (the bytes past `live` hold whatever they hold)
            std::memcpy(old, same.id, 16);
            check_chunk(enc, old, lut, c0, live, 100 + kind);
            {
                uint32_t ew[12], ow[4], nw[4];
                for (int j = 0; j < 12; ++j) ew[j] = word_at(enc + 4 * j);
                for (int j = 0; j < 4; ++j) ow[j] = word_at(old + 4 * j);
                CHECK(dirty_chunk(ew, ow, lut, c0, live, nw) == 0, "equal ids are clean", kind, c0, live);
            }
            // one differing byte, by 0x01 / 0x7F / 0x80 / 0xFF, at every position (past `live` it must not count)
            for (int i = 0; i < 16; ++i) for (int f = 0; f < 4; ++f) {
                std::memcpy(old, same.id, 16);
                old[i] ^= flips[f];
                check_chunk(enc, old, lut, c0, live, 200 + kind);
            }
            // random old ids, and old ids that differ everywhere
            for (int i = 0; i < 16; ++i) old[i] = (uint8_t)rnd();
            check_chunk(enc, old, lut, c0, live, 300 + kind);
            for (int i = 0; i < 16; ++i) old[i] = (uint8_t)(same.id[i] ^ flips[rnd() & 3]);
            check_chunk(enc, old, lut, c0, live, 400 + kind);
            // a changed encoding with an unchanged id is not dirty: the old ids are those of `enc`, the new encoding differs in every
            // cell; under the shared lut many of its ids are the old ones, and the bits must follow the ids, not the encodings
            std::memcpy(old, same.id, 16);
            for (int i = 0; i < 16; ++i) do draw_cell(enc2 + 3 * i); while (std::memcmp(enc2 + 3 * i, enc + 3 * i, 3) == 0);
            check_chunk(enc2, old, lut, c0, live, 500 + kind);
            if (kind == LUT_SHARED) {
                // ... and with the same key class in every cell (key + 6 keeps key % 3 and key % 2) nothing is dirty at all
                for (int i = 0; i < 16; ++i) { enc[3 * i] = (uint8_t)(rnd() & 1); enc[3 * i + 1] = (uint8_t)(rnd() % 6); enc[3 * i + 2] = (uint8_t)(rnd() & 3); }
                const RefChunk base = ref_chunk(enc, enc, lut, c0, 16);
                std::memcpy(old, base.id, 16);
                std::memcpy(enc2, enc, 48);
                for (int i = 0; i < 16; ++i) enc2[3 * i] = (uint8_t)(enc[3 * i] + 6);        // type + 6 <= 7: key + 6
                uint32_t ew[12], ow[4], nw[4];
                for (int j = 0; j < 12; ++j) ew[j] = word_at(enc2 + 4 * j);
                for (int j = 0; j < 4; ++j) ow[j] = word_at(old + 4 * j);
                CHECK(dirty_chunk(ew, ow, lut, c0, live, nw) == 0, "changed encodings, unchanged ids", c0, live);
                check_chunk(enc2, old, lut, c0, live, 600);
            }
            if (kind == LUT_AGENT_DIFFERS) {
                // the agent's table is used at cell 27 and nowhere else: against ids taken from the plain table alone, exactly the
                // agent's cell (where it is live) is dirty
                for (int i = 0; i < 16; ++i) old[i] = lut[enc[3 * i] | (enc[3 * i + 1] << 3) | (enc[3 * i + 2] << 6)];
                uint32_t ew[12], ow[4], nw[4];
                for (int j = 0; j < 12; ++j) ew[j] = word_at(enc + 4 * j);
                for (int j = 0; j < 4; ++j) ow[j] = word_at(old + 4 * j);
                const int ia = (AGENT_ - c0 + CELLS_) % CELLS_;
                CHECK(dirty_chunk(ew, ow, lut, c0, live, nw) == (ia < live ? 1u << ia : 0u), "the agent's table at cell 27 only", c0, live, ia);
            }
        }
    }
}

int main() {
    test_flags();
    test_keys();
    test_agent_and_split();
    test_chunks();
    if (failures) { std::printf("%ld of %ld checks failed\n", failures, checks); return 1; }
    std::printf("ok %ld checks\n", checks);
    return 0;
}
