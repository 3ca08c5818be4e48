// Stand-alone replay of the step-digest fixture on the host build of the engine's headers (tests/test_step_digest_sanitized.py compiles
// this file plain and with sanitizers and runs it directly; nothing of it is loaded into Python).
//
//   step_digest_host IN OUT
//
// IN  (written by the test):  u32 magic, u32 sizeof(LevelCfg), u32 kinds;  per kind: LevelCfg, u32 steps, u32 streams, u32 lane (1: a second
//                             pass with the lane generator, hs_generate_lane, making every level), u64 seeds[streams], u8 actions[steps][streams].
// OUT per kind and pass:      u8 first_image[streams][147], u8 first_dir[streams], u8 image[steps][streams][147], u8 dir[steps][streams],
//                             f64 reward[steps][streams], u8 done[steps][streams], u8 suggestion[steps][streams] (255: the expert is dead).
//
// Every stream is generated, stepped in k_step's order of operations (step_env_prefetch) with auto-reset, and the expert (bot_decide, eager
// search, a fresh state per episode) is consulted before every step and told the action that was taken.
#include "hostsim/hostsim.cpp"

#include <cstdio>
#include <vector>

static const uint32_t MAGIC = 0x53444947u;

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

static int new_episode(const LevelCfg& cfg, bool lane, uint32_t* mt, int32_t* mti, uint8_t* rec, Hot* hot, uint64_t* stale, uint8_t* image, uint8_t* dir) {
    if (!lane) {
        batch_new_episode(&cfg, mt, mti, rec, hot, stale, nullptr, image, dir);
        return 0;
    }
    if (hs_generate_lane(&cfg, mt, mti, rec, hot) < 0) return -1;
    *stale = 0;
    hs_observe(&cfg, rec, hot, image);
    *dir = hot->dir;
    hs_start_carry(&cfg, rec, hot, stale);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t head[3];
    if (!rd(in, head, sizeof(head)) || head[0] != MAGIC || head[1] != sizeof(LevelCfg)) { fprintf(stderr, "bad header\n"); return 2; }
    hs_bot_set_eager(1);
    const int stack_cap = 1024;       // room for any subgoal stack these streams can build: the reference's list is unbounded (the default is 48)
    long long steps_run = 0, consulted = 0;
    for (uint32_t k = 0; k < head[2]; ++k) {
        LevelCfg cfg;
        uint32_t dims[3];
        if (!rd(in, &cfg, sizeof(cfg)) || !rd(in, dims, sizeof(dims))) { fprintf(stderr, "kind %u: short input\n", k); return 2; }
        const size_t T = dims[0], S = dims[1];
        const bool with_lane = dims[2] != 0;
        if (T == 0 || S == 0 || T > 4096 || S > 4096 || cfg.rec_bytes <= 0 || cfg.rec_bytes > 4096) { fprintf(stderr, "kind %u: bad sizes\n", k); return 2; }
        std::vector<uint64_t> seeds(S);
        std::vector<uint8_t> actions(T * S);
        if (!rd(in, seeds.data(), S * 8) || !rd(in, actions.data(), T * S)) { fprintf(stderr, "kind %u: short input\n", k); return 2; }
        for (int pass = 0; pass < (with_lane ? 2 : 1); ++pass) {
            std::vector<uint8_t> first_image(S * OBS_BYTES), first_dir(S), image(T * S * OBS_BYTES), dir(T * S), done(T * S), sug(T * S, 255);
            std::vector<double> reward(T * S);
            std::vector<uint32_t> mt(MT_N);
            std::vector<uint8_t> rec(cfg.rec_bytes), bot(hs_bot_state_bytes(stack_cap));
            for (size_t i = 0; i < S; ++i) {
                hs_seed(seeds[i], mt.data());
                int32_t mti = MT_N;
                Hot hot;
                memset(&hot, 0, sizeof(hot));
                hot.last_locked = NONE8;
                uint64_t stale = 0;
                if (new_episode(cfg, pass == 1, mt.data(), &mti, rec.data(), &hot, &stale, &first_image[i * OBS_BYTES], &first_dir[i]) < 0) {
                    fprintf(stderr, "kind %u stream %zu: the lane generator failed\n", k, i);
                    return 3;
                }
                std::fill(bot.begin(), bot.end(), 0);
                bool first = true, alive = true;
                int last = -1;
                for (size_t t = 0; t < T; ++t) {
                    const size_t at = t * S + i;
                    if (alive) {
                        const int a = hs_bot_decide(&cfg, rec.data(), &hot, &stale, bot.data(), stack_cap, first ? 1 : 0, last);
                        ++consulted;
                        sug[at] = (uint8_t)a;
                        alive = a != 255;
                        first = false;
                    }
                    last = actions[at];
                    double rw = 0.0;
                    const int d = hs_step64_prefetch(&cfg, rec.data(), &hot, &stale, last, &rw, nullptr);
                    ++steps_run;
                    reward[at] = rw;
                    done[at] = d ? 1 : 0;
                    if (d) {
                        if (new_episode(cfg, pass == 1, mt.data(), &mti, rec.data(), &hot, &stale, &image[at * OBS_BYTES], &dir[at]) < 0) {
                            fprintf(stderr, "kind %u stream %zu step %zu: the lane generator failed\n", k, i, t);
                            return 3;
                        }
                        std::fill(bot.begin(), bot.end(), 0);
                        first = true; alive = true; last = -1;
                    } else {
                        hs_observe(&cfg, rec.data(), &hot, &image[at * OBS_BYTES]);
                        dir[at] = hot.dir;
                    }
                }
            }
            bool ok = fwrite(first_image.data(), 1, first_image.size(), out) == first_image.size();
            ok = ok && fwrite(first_dir.data(), 1, S, out) == S;
            ok = ok && fwrite(image.data(), 1, image.size(), out) == image.size();
            ok = ok && fwrite(dir.data(), 1, T * S, out) == T * S;
            ok = ok && fwrite(reward.data(), 8, T * S, out) == T * S;
            ok = ok && fwrite(done.data(), 1, T * S, out) == T * S;
            ok = ok && fwrite(sug.data(), 1, T * S, out) == T * S;
            if (!ok) { fprintf(stderr, "kind %u: short write\n", k); return 2; }
        }
    }
    if (fclose(out) != 0) return 2;
    fclose(in);
    printf("ok %lld steps %lld decisions\n", steps_run, consulted);
    return 0;
}
