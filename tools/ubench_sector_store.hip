// ubench_sector_store.hip -- do partial-line stores cost only their own bytes?  (experiment tool)
//
// The delta render stores the parts of 1 048 576 x 9408-byte frames whose cells changed.  This program stores such parts of a 9.9 GB
// buffer at a piece granularity P of 128 (whole lines: the line rule), 64, 32 or 16 bytes, driven by per-env 49-bit dirty masks, and
// prints one JSON line per (masks, P): ms (median of --reps launches), bytes stored, bytes stored per us, and the time relative to
// P = 128 on the same masks.  A plain non-temporal fill of the same buffer, in the same process, is the ceiling.
//   * pieces are tested one lane each over the flat buffer (a piece of 128 bytes can span two envs: 9408 = 73.5 lines); a wave compacts
//     its dirty pieces by a ballot into its own LDS list and stores them 16 bytes per lane, non-temporal, consecutive lanes on
//     consecutive chunks -- the store shape of the render's kernels;
//   * masks: "clean" (none dirty: the cost of the tests alone), "mix" (a synthetic mixture near the measured BossLevel one:
//     60 % clean envs, the rest with 6-40 dirty cells in whole view columns and rows, as turns and moves leave them), "u<f>" (every
//     cell dirty with probability f).
// WRITE_SIZE / FETCH_SIZE: run it under `rocprofv3 --pmc WRITE_SIZE` and, in a run of its own, `--pmc FETCH_SIZE` (a FETCH_SIZE that
// rises with smaller pieces would mean read-modify-write on the memory side).
//   hipcc --offload-arch=gfx950 -O3 -o tools/ubench_sector_store tools/ubench_sector_store.hip && tools/ubench_sector_store [reps]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int VIEW = 7, PIX_BYTES = 9408, PERIOD = 2 * PIX_BYTES;      // two envs: a whole number of 128-byte lines
constexpr int64_t N_ENVS = 1048576;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// cells of one env that bytes [s, t) of its image come from (8-byte chunks; 24-byte tile rows at a 168-byte pitch)
static uint64_t cells_of(int s, int t) {
    uint64_t m = 0;
    for (int b = s; b < t; b += 8) {
        const int ch = b >> 3, py = ch / 21, cx = ch - py * 21;
        m |= 1ull << ((cx / 3) * VIEW + (py >> 3));
    }
    return m;
}

// per piece of a two-env period: cells of the first env it touches (ma) and of the next one (mb); eo = which env of the period it starts in
struct PieceCells { uint64_t ma, mb; uint32_t eo, pad; };

template <int P>
__global__ __launch_bounds__(512) void k_store(int64_t n, uint8_t* __restrict__ buf, const uint64_t* __restrict__ mask, const PieceCells* __restrict__ tab) {
    constexpr int NPER = PERIOD / P, S = P / 16;
    __shared__ PieceCells s_tab[NPER];
    __shared__ uint32_t s_wl[8][64];
    for (int i = threadIdx.x; i < NPER; i += 512) s_tab[i] = tab[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t npieces = n * PIX_BYTES / P;
    const int64_t nw = (int64_t)gridDim.x * 8;
    for (int64_t q0 = ((int64_t)blockIdx.x * 8 + wave) * 64; q0 < npieces; q0 += nw * 64) {
        const int64_t q = q0 + lane;
        bool d = false;
        if (q < npieces) {
            const int64_t per = q / NPER;
            const PieceCells pc = s_tab[q - per * NPER];
            const int64_t ea = per * 2 + pc.eo;
            d = (mask[ea] & pc.ma) != 0 || (pc.mb && ea + 1 < n && (mask[ea + 1] & pc.mb) != 0);
        }
        const uint64_t b = __ballot(d);
        if (!b) continue;
        if (d) s_wl[wave][__builtin_popcountll(b & ((1ull << lane) - 1))] = (uint32_t)lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int cnt = __builtin_popcountll(b);
        u32x4* out = (u32x4*)(buf + q0 * P);
        for (int i = lane; i < cnt * S; i += 64) {
            const int k = (int)s_wl[wave][i / S] * S + (i & (S - 1));
            const uint32_t v = (uint32_t)(q0 * S + k);
            __builtin_nontemporal_store((u32x4){v, v ^ 0x5a5a5a5au, v + 1u, ~v}, out + k);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

__global__ __launch_bounds__(512) void k_fill(int64_t nvec, u32x4* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 512 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 512) {
        const uint32_t v = (uint32_t)i;
        __builtin_nontemporal_store((u32x4){v, v, v, v}, out + i);
    }
}

static std::vector<PieceCells> table(int P) {
    std::vector<PieceCells> t(PERIOD / P);
    for (int i = 0; i < PERIOD / P; ++i) {
        const int b0 = i * P, b1 = b0 + P, ea = b0 / PIX_BYTES, eb = (b1 - 1) / PIX_BYTES, s = b0 - ea * PIX_BYTES;
        t[i].eo = (uint32_t)ea;
        t[i].ma = cells_of(s, eb != ea ? PIX_BYTES : b1 - ea * PIX_BYTES);
        t[i].mb = eb != ea ? cells_of(0, b1 - eb * PIX_BYTES) : 0;
        t[i].pad = 0;
    }
    return t;
}

static std::vector<uint64_t> masks(const std::string& kind, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<uint64_t> m(N_ENVS, 0);
    if (kind == "clean") return m;
    if (kind[0] == 'u') {
        const double f = atof(kind.c_str() + 1);
        for (auto& x : m)
            for (int c = 0; c < 49; ++c) x |= (u(rng) < f ? 1ull : 0ull) << c;
        return m;
    }
    // mix: 60 % clean; else 6-40 dirty cells, grown as whole view columns (x) / rows (y) of the 7x7 view from a random start
    for (auto& x : m) {
        if (u(rng) < 0.6) continue;
        const int want = 6 + (int)(u(rng) * 35);
        const bool cols = u(rng) < 0.5;
        int line = (int)(u(rng) * VIEW), got = 0;
        while (got < want) {
            const int from = (int)(u(rng) * 3), to = VIEW - (int)(u(rng) * 2);
            for (int k = from; k < to && got < want; ++k) {
                const int c = cols ? line * VIEW + k : k * VIEW + line;
                if (!(x >> c & 1)) { x |= 1ull << c; ++got; }
            }
            line = (line + 1) % VIEW;
        }
    }
    return m;
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 7;
    int dev = 0, cus = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const size_t bytes = (size_t)N_ENVS * PIX_BYTES;
    uint8_t* buf = nullptr;
    uint64_t* dmask = nullptr;
    PieceCells* dtab = nullptr;
    CK(hipMalloc((void**)&buf, bytes));
    CK(hipMalloc((void**)&dmask, N_ENVS * 8));
    CK(hipMalloc((void**)&dtab, sizeof(PieceCells) * (PERIOD / 16)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const unsigned blocks = (unsigned)cus * 3;
    auto timed = [&](auto launch) {
        launch();
        CK(hipDeviceSynchronize());
        std::vector<float> ms;
        for (int r = 0; r < reps; ++r) {
            CK(hipEventRecord(e0));
            launch();
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float t = 0;
            CK(hipEventElapsedTime(&t, e0, e1));
            ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        return (double)ms[ms.size() / 2];
    };
    const double fill = timed([&] { hipLaunchKernelGGL(k_fill, dim3(cus * 4), dim3(512), 0, 0, (int64_t)(bytes / 16), (u32x4*)buf); });
    printf("{\"kind\": \"fill\", \"ms\": %.4f, \"bytes\": %zu, \"bytes_per_us\": %.0f}\n", fill, bytes, bytes / (fill * 1e3));
    const char* kinds[] = {"clean", "mix", "u0.05", "u0.1", "u0.2", "u0.4"};
    const int pieces[] = {128, 64, 32, 16};
    for (const char* kind : kinds) {
        const std::vector<uint64_t> m = masks(kind, 1234);
        CK(hipMemcpy(dmask, m.data(), N_ENVS * 8, hipMemcpyHostToDevice));
        double t128 = 0;
        for (int P : pieces) {
            const std::vector<PieceCells> t = table(P);
            CK(hipMemcpy(dtab, t.data(), sizeof(PieceCells) * t.size(), hipMemcpyHostToDevice));
            // bytes this P stores (host count over the same table)
            double stored = 0;
            for (int64_t per = 0; per < N_ENVS / 2; ++per)
                for (const PieceCells& pc : t)
                    if ((m[per * 2 + pc.eo] & pc.ma) || (pc.mb && (m[per * 2 + pc.eo + 1] & pc.mb))) stored += P;
            double ms = 0;
            switch (P) {
                case 128: ms = timed([&] { hipLaunchKernelGGL(k_store<128>, dim3(blocks), dim3(512), 0, 0, N_ENVS, buf, dmask, dtab); }); break;
                case 64: ms = timed([&] { hipLaunchKernelGGL(k_store<64>, dim3(blocks), dim3(512), 0, 0, N_ENVS, buf, dmask, dtab); }); break;
                case 32: ms = timed([&] { hipLaunchKernelGGL(k_store<32>, dim3(blocks), dim3(512), 0, 0, N_ENVS, buf, dmask, dtab); }); break;
                default: ms = timed([&] { hipLaunchKernelGGL(k_store<16>, dim3(blocks), dim3(512), 0, 0, N_ENVS, buf, dmask, dtab); }); break;
            }
            CK(hipGetLastError());
            if (P == 128) t128 = ms;
            printf("{\"kind\": \"%s\", \"P\": %d, \"ms\": %.4f, \"bytes\": %.0f, \"bytes_per_env\": %.1f, \"bytes_per_us\": %.0f, \"vs_128\": %.3f}\n",
                   kind, P, ms, stored, stored / N_ENVS, stored / (ms * 1e3), ms / t128);
            fflush(stdout);
        }
    }
    CK(hipFree(buf));
    CK(hipFree(dmask));
    CK(hipFree(dtab));
    return 0;
}
