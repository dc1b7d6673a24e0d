// What the host kernel drivers share (tests/kin_host_driver.cpp, tests/site_host_driver.cpp): the definitions behind
// tests/host_kernel/hip/hip_runtime.h, the launcher, the generator and the panels.  Include it once, after <hip/hip_runtime.h> and
// snpm_k_common.hpp (pk_off, WAVE); a driver is one translation unit with its own main.
#pragma once
#include <pthread.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

using namespace snpm;

constexpr int HK_MAX_THREADS = 1024;        // threads of a block, at most
thread_local host_dim3 threadIdx, blockIdx, gridDim;
static pthread_barrier_t g_block_bar, g_wave_bar[HK_MAX_THREADS / WAVE];
static uint32_t g_xchg[HK_MAX_THREADS / WAVE][2][WAVE];
static thread_local unsigned t_exchanges;

void __syncthreads() { pthread_barrier_wait(&g_block_bar); }

// every lane's value of this exchange, by lane.  Two buffers, one barrier per exchange: a thread that is already writing exchange
// n + 1 cannot disturb one still reading exchange n - 1, because every thread of the wave finished that read before it entered
// the barrier of exchange n
static const uint32_t *wave_exchange(uint32_t value)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, buf = t_exchanges++ & 1;
    g_xchg[wave][buf][lane] = value;
    pthread_barrier_wait(&g_wave_bar[wave]);
    return g_xchg[wave][buf];
}

unsigned long long __ballot(int predicate)
{
    const uint32_t *all = wave_exchange(predicate != 0);
    unsigned long long m = 0;
    for (int l = 0; l < WAVE; ++l) m |= (unsigned long long)all[l] << l;
    return m;
}

uint32_t __shfl_xor(uint32_t value, int lane_mask) { return wave_exchange(value)[(threadIdx.x & 63) ^ lane_mask]; }

struct Launch {
    unsigned gx, gy;
    std::function<void()> body;
};
static Launch g_launch;

static void *thread_main(void *arg)
{
    threadIdx = {(unsigned)(intptr_t)arg, 0, 0};
    gridDim = {g_launch.gx, g_launch.gy, 1};
    for (unsigned by = 0; by < g_launch.gy; ++by)
        for (unsigned bx = 0; bx < g_launch.gx; ++bx) {
            blockIdx = {bx, by, 0};
            g_launch.body();
            pthread_barrier_wait(&g_block_bar);          // the next block reuses the `__shared__` statics
        }
    return nullptr;
}

// a grid of gx x gy blocks of `threads` threads (whole waves), one real thread per GPU thread
static void launch(int threads, unsigned gx, unsigned gy, std::function<void()> body)
{
    if (threads <= 0 || threads > HK_MAX_THREADS || threads % WAVE) { fprintf(stderr, "launch: %d threads\n", threads); exit(3); }
    g_launch = {gx, gy, body};
    pthread_barrier_init(&g_block_bar, nullptr, (unsigned)threads);
    for (int w = 0; w < threads / WAVE; ++w) pthread_barrier_init(&g_wave_bar[w], nullptr, WAVE);
    std::vector<pthread_t> th((size_t)threads);
    for (int t = 0; t < threads; ++t)
        if (pthread_create(&th[(size_t)t], nullptr, thread_main, (void *)(intptr_t)t)) { perror("pthread_create"); exit(3); }
    for (int t = 0; t < threads; ++t) pthread_join(th[(size_t)t], nullptr);
    for (int w = 0; w < threads / WAVE; ++w) pthread_barrier_destroy(&g_wave_bar[w]);
    pthread_barrier_destroy(&g_block_bar);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// a heap block of exactly `bytes` bytes at the alignment of a device allocation: the sanitizer sees every byte past it
static void *exact_block(size_t bytes)
{
    void *p = nullptr;
    if (posix_memalign(&p, 256, bytes ? bytes : 1)) { perror("posix_memalign"); exit(3); }
    return p;
}

// TIGHT: int8 rows of exactly n_acc bytes, whatever the pitch policy
enum Layout { INT8, PACKED, SPLIT, TIGHT };

struct PanelStyle {
    bool library_pitch;     // the pitches of the library: int8 rows padded to 128 bytes, packed whole rows to 256, split rows = whole
                            // 256-byte blocks + a power-of-two tail; else rows of exactly their bytes (split: whole 64-byte blocks + tail)
    bool random_pad;        // pad bytes, fields past n_acc and the value of a missing int8 call: anything; else 0xFF / missing
    bool blank_accession;   // accession 1 of a panel of more than two has no call
};

// a panel of exactly the bytes its layout needs; calls[r * n_acc + a] keeps the values (-1 / 0 / 1 / 2, int8 panels also 3)
struct Panel {
    int8_t *d = nullptr;
    int64_t pitch = 0, desc = 0, n_snp = 0, n_acc = 0;
    bool packed = false;
    std::vector<int8_t> calls;
};

static Panel make_panel(Layout lay, int64_t n_snp, int64_t n_acc, const PanelStyle &style)
{
    Panel p;
    p.n_snp = n_snp; p.n_acc = n_acc;
    p.packed = lay == PACKED || lay == SPLIT;
    p.calls.resize((size_t)(n_snp * n_acc));
    for (auto &c : p.calls) {
        const uint32_t u = rnd() % 100;
        c = (int8_t)(u < 12 ? -1 : u < 55 ? 0 : u < 88 ? 1 : (u < 96 || p.packed) ? 2 : 3);
    }
    for (int64_t r = 0; r < n_snp && style.blank_accession && n_acc > 2; ++r) p.calls[(size_t)(r * n_acc + 1)] = -1;
    const int64_t row_bytes = p.packed ? (n_acc + 3) / 4 : n_acc;
    size_t bytes;
    if (lay == SPLIT) {                     // main part: the whole blocks of a row; tail: the rest, rows of 2^t bytes
        const int64_t block = style.library_pitch ? 256 : 64, main = row_bytes / block * block;
        int64_t tail = 4;
        int lg = 2;
        while (tail < row_bytes - main) tail <<= 1, ++lg;
        const int64_t tail_off = (n_snp * main + 255) / 256 * 256;
        p.pitch = main;
        p.desc = 1 | ((int64_t)(lg + 1) << 1) | ((tail_off / 256) << 8);
        bytes = (size_t)(tail_off + n_snp * tail);
    } else {
        const int64_t unit = !style.library_pitch || lay == TIGHT ? 1 : p.packed ? 256 : 128;
        p.pitch = (row_bytes + unit - 1) / unit * unit;
        p.desc = p.packed ? 1 : 0;
        bytes = (size_t)(n_snp * p.pitch);
    }
    p.d = (int8_t *)exact_block(bytes);
    for (size_t i = 0; i < bytes; ++i) p.d[i] = style.random_pad ? (int8_t)rnd() : (int8_t)0xFF;
    for (int64_t r = 0; r < n_snp; ++r)
        for (int64_t b = 0; b < row_bytes; ++b) {
            if (!p.packed) {
                const int8_t c = p.calls[(size_t)(r * n_acc + b)];
                p.d[r * p.pitch + b] = c >= 0 ? c : style.random_pad ? (int8_t)(0x80 | (rnd() & 0x7F)) : (int8_t)0xFF;
                continue;
            }
            unsigned out = 0;
            for (int f = 0; f < 4; ++f) {
                const int64_t a = 4 * b + f;
                const int v = a < n_acc ? p.calls[(size_t)(r * n_acc + a)] : style.random_pad ? (int)(rnd() & 3) - 1 : -1;
                out |= (unsigned)(v < 0 ? 3 : v) << (2 * f);
            }
            ((uint8_t *)p.d)[pk_off(p.pitch, p.desc, r, b)] = (uint8_t)out;
        }
    return p;
}
