// The kernel source of csrc/snpm_k_site.hpp compiled for the host (tests/site_host_shim/hip/hip_runtime.h stands in for the HIP
// header) and run with its launch geometry: every block by 512 real threads with a barrier for __syncthreads, the shuffles of a wave
// through its 64 threads.  Built with -fsanitize=address,undefined by tests/test_sitestats_cpu.py and run as a child process: the
// panel, the row list, the membership words and the slab's counts are heap blocks of exactly the size the library would use, the
// pad bytes of the rows hold arbitrary values and the workspace starts with stale contents.  Every count is compared with a
// brute-force count.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <pthread.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "snpm_k_common.hpp"
#include "snpm_k_site.hpp"

using namespace snpm;

thread_local site_dim3 threadIdx, blockIdx, gridDim;
static pthread_barrier_t g_block_bar, g_wave_bar[SITE_THREADS / WAVE];
static uint32_t g_val[SITE_THREADS / WAVE][2][WAVE];
static thread_local unsigned t_shuffles;

void __syncthreads() { pthread_barrier_wait(&g_block_bar); }

// two buffers, one barrier per shuffle: a thread that is already writing shuffle n + 1 cannot disturb one still reading shuffle
// n - 1, because every thread of the wave finished that read before it entered the barrier of shuffle n
uint32_t __shfl_xor(uint32_t value, int lane_mask)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, buf = t_shuffles++ & 1;
    g_val[wave][buf][lane] = value;
    pthread_barrier_wait(&g_wave_bar[wave]);
    return g_val[wave][buf][lane ^ lane_mask];
}

struct Launch {
    unsigned gx;
    std::function<void()> body;
};
static Launch g_launch;

static void *thread_main(void *arg)
{
    threadIdx = {(unsigned)(intptr_t)arg, 0, 0};
    gridDim = {g_launch.gx, 1, 1};
    for (unsigned bx = 0; bx < g_launch.gx; ++bx) {
        blockIdx = {bx, 0, 0};
        g_launch.body();
        pthread_barrier_wait(&g_block_bar);              // the next block reuses the `__shared__` statics
    }
    return nullptr;
}

static void launch(unsigned gx, std::function<void()> body)
{
    g_launch = {gx, body};
    pthread_t th[SITE_THREADS];
    for (int t = 0; t < SITE_THREADS; ++t)
        if (pthread_create(&th[t], nullptr, thread_main, (void *)(intptr_t)t)) { perror("pthread_create"); exit(3); }
    for (int t = 0; t < SITE_THREADS; ++t) pthread_join(th[t], nullptr);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// INT8 / PACKED / SPLIT: the pitches of the library (int8 rows padded to 128 bytes, packed whole rows to 256, split rows = whole
// 256-byte blocks + a power-of-two tail); TIGHT: int8 rows of exactly n_acc bytes (no wide loads unless n_acc is a multiple of 16)
enum Layout { INT8, PACKED, SPLIT, TIGHT };

static void *exact_block(size_t bytes)
{
    void *p = nullptr;
    if (posix_memalign(&p, 256, bytes ? bytes : 1)) { perror("posix_memalign"); exit(3); }
    return p;
}

// a panel of exactly the bytes its layout needs; calls[r * n_acc + a] keeps the values (-1 / 0 / 1 / 2, int8 panels also 3)
struct Panel {
    int8_t *d = nullptr;
    int64_t pitch = 0, desc = 0, n_snp = 0, n_acc = 0;
    bool packed = false;
    std::vector<int8_t> calls;
};

static Panel make_panel(Layout lay, int64_t n_snp, int64_t n_acc)
{
    Panel p;
    p.n_snp = n_snp; p.n_acc = n_acc;
    p.packed = lay == PACKED || lay == SPLIT;
    p.calls.resize((size_t)(n_snp * n_acc));
    for (auto &c : p.calls) {
        const uint32_t u = rnd() % 100;
        c = (int8_t)(u < 12 ? -1 : u < 55 ? 0 : u < 85 ? 1 : (u < 95 || p.packed) ? 2 : 3);
    }
    size_t bytes;
    if (!p.packed) {
        p.pitch = lay == TIGHT ? n_acc : (n_acc + 127) / 128 * 128;
        bytes = (size_t)(n_snp * p.pitch);
        p.d = (int8_t *)exact_block(bytes);
        for (size_t i = 0; i < bytes; ++i) p.d[i] = (int8_t)rnd();                      // pad bytes: anything
        for (int64_t r = 0; r < n_snp; ++r)
            for (int64_t a = 0; a < n_acc; ++a) {
                const int8_t c = p.calls[(size_t)(r * n_acc + a)];
                p.d[r * p.pitch + a] = c < 0 ? (int8_t)(0x80 | (rnd() & 0x7F)) : c;       // missing: any negative value
            }
        return p;
    }
    const int64_t row_bytes = (n_acc + 3) / 4;
    int64_t tail = 0, tail_off = 0;
    if (lay == SPLIT) {
        const int64_t main = row_bytes / 256 * 256, rem = row_bytes - main;
        tail = 4;
        while (tail < rem) tail <<= 1;
        p.pitch = main;
        tail_off = (n_snp * main + 255) / 256 * 256;
        int lg = 0;
        while (((int64_t)1 << lg) < tail) ++lg;
        p.desc = 1 | ((int64_t)(lg + 1) << 1) | ((tail_off / 256) << 8);
        bytes = (size_t)(tail_off + n_snp * tail);
    } else {
        p.pitch = (row_bytes + 255) / 256 * 256;
        p.desc = 1;
        bytes = (size_t)(n_snp * p.pitch);
    }
    p.d = (int8_t *)exact_block(bytes);
    for (size_t i = 0; i < bytes; ++i) p.d[i] = (int8_t)rnd();
    for (int64_t r = 0; r < n_snp; ++r)
        for (int64_t b = 0; b < row_bytes; ++b) {
            unsigned out = 0;
            for (int f = 0; f < 4; ++f) {
                const int64_t a = 4 * b + f;
                const int v = a < n_acc ? p.calls[(size_t)(r * n_acc + a)] : (int)(rnd() & 3) - 1;     // fields past n_acc: anything
                out |= (unsigned)(v < 0 ? 3 : v) << (2 * f);
            }
            ((uint8_t *)p.d)[pk_off(p.pitch, p.desc, r, b)] = (uint8_t)out;
        }
    return p;
}

static int g_fails = 0;

// the groups of a case as bitmasks over the panel's columns: 1 = all accessions; 2 = one column, a subset; 3 = a subset, an empty
// group, a subset that overlaps the first; more = subsets with group 5 empty and group 6 of one column
static std::vector<uint32_t> make_groups(int n_groups, int64_t n_acc)
{
    const int64_t nwords = (n_acc + 31) / 32;
    std::vector<uint32_t> m((size_t)(n_groups * nwords), 0u);
    auto set = [&](int g, int64_t c) { m[(size_t)(g * nwords + (c >> 5))] |= 1u << (c & 31); };
    for (int g = 0; g < n_groups; ++g) {
        const bool all = n_groups == 1, empty = (n_groups == 3 && g == 1) || (n_groups > 3 && g == 5);
        const bool one = (n_groups == 2 && g == 0) || (n_groups > 3 && g == 6);
        if (empty) continue;
        if (one) { set(g, (int64_t)(rnd() % n_acc)); continue; }
        for (int64_t c = 0; c < n_acc; ++c)
            if (all || rnd() % 3 != 0) set(g, c);
        if (n_groups == 3 && g == 2) set(g, 0), set(0, 0);          // the first and the last group share column 0 for sure
    }
    return m;
}

// what snpm_panel_site_counts does after its validation, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int n_groups, int use_rows, int64_t n_rows, size_t ws_bytes)
{
    Panel p = make_panel(lay, n_snp, n_acc);
    const int64_t nwords = (n_acc + 31) / 32;
    const std::vector<uint32_t> groups = make_groups(n_groups, n_acc);
    uint32_t *member = (uint32_t *)exact_block(groups.size() * sizeof(uint32_t));
    memcpy(member, groups.data(), groups.size() * sizeof(uint32_t));
    int64_t row0 = 0, *rows = nullptr;
    if (use_rows) {                         // unsorted, with repeats
        rows = (int64_t *)exact_block((size_t)n_rows * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = (int64_t)(rnd() % n_snp);
        if (n_rows > 2) rows[n_rows - 1] = rows[0];
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    int32_t *counts = (int32_t *)exact_block((size_t)(n_groups * n_rows) * 16);
    memset(counts, 0x5A, (size_t)(n_groups * n_rows) * 16);
    int lg_s = 0, cpl = 0, slabs = 0;
    if (!site_geometry(n_acc, p.packed, &lg_s, &cpl)) { printf("case %s: panel too wide\n", name); ++g_fails; return; }
    const bool wide = site_wide_rows(p.d, p.pitch, p.desc);
    if (n_rows > 0) {
        int64_t slab_rows = std::max<int64_t>(64, (int64_t)(ws_bytes / (size_t)(16 * n_groups)) / 64 * 64);
        slab_rows = std::min(slab_rows, n_rows);
        const size_t out_bytes = (size_t)(n_groups * slab_rows) * 16;
        int32_t *ws = (int32_t *)exact_block(out_bytes);
        memset(ws, 0xA5, out_bytes);                                  // stale contents
        const int rpw = WAVE >> lg_s, waves = SITE_THREADS / WAVE;
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab, as in the library
            int64_t *slab_list = nullptr;
            if (rows) {
                slab_list = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(slab_list, rows + s0, (size_t)n_valid * sizeof(int64_t));
            }
            const int64_t batches = (n_valid + rpw - 1) / rpw;
            const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((batches + waves - 1) / waves, 2));     // two blocks: the stride loop runs
            launch(grid, [&] {
                if (p.packed) {
                    if (wide) k_site_counts<true, true>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                    else k_site_counts<true, false>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                } else {
                    if (wide) k_site_counts<false, true>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                    else k_site_counts<false, false>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                }
            });
            for (int g = 0; g < n_groups; ++g) memcpy(counts + (g * n_rows + s0) * 4, ws + g * n_valid * 4, (size_t)n_valid * 16);
            free(slab_list);
        }
        free(ws);
    }
    long bad = 0;
    for (int g = 0; g < n_groups; ++g)
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t prow = rows ? rows[r] : row0 + r;
            int32_t want[4] = {0, 0, 0, 0};
            for (int64_t c = 0; c < n_acc; ++c) {
                if (!((groups[(size_t)(g * nwords + (c >> 5))] >> (c & 31)) & 1u)) continue;
                const int v = p.calls[(size_t)(prow * n_acc + c)];
                if (v >= 0 && v <= 2) ++want[v];
                want[3] += v >= 0;
            }
            bad += memcmp(want, counts + (g * n_rows + r) * 4, 16) != 0;
        }
    printf("case %s layout=%d acc=%lld groups=%d rows=%lld lanes=%d chunks=%d wide=%d slabs=%d %s\n", name, (int)lay, (long long)n_acc, n_groups,
           (long long)n_rows, 1 << lg_s, cpl, (int)wide, slabs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(counts); free(rows); free(member); free(p.d);
}

int main()
{
    pthread_barrier_init(&g_block_bar, nullptr, SITE_THREADS);
    for (auto &b : g_wave_bar) pthread_barrier_init(&b, nullptr, WAVE);
    const size_t big = size_t(256) << 20;
    const int group_counts[4] = {1, 2, 3, SNPM_SITE_MAX_GROUPS};
    int k = 0;
    for (int64_t acc : {1, 2, 31, 32, 33, 63, 64, 65, 130, 1135})
        for (int64_t rows : {0, 1, 63, 64, 65}) {
            const Layout lay = (Layout)(k % 3);
            run_case("small", lay, rows + 3, acc, group_counts[(k / 3) % 4], 0, rows, big);
            ++k;
        }
    // the width of the 1001-Genomes panel in every layout (split: 256 + 32 bytes per row), with every group count
    run_case("1135-int8", INT8, 70, 1135, 3, 0, 65, big);
    run_case("1135-packed", PACKED, 70, 1135, SNPM_SITE_MAX_GROUPS, 0, 65, big);
    run_case("1135-split", SPLIT, 70, 1135, 2, 0, 65, big);
    run_case("1135-split-all", SPLIT, 70, 1135, 1, 0, 64, big);
    // rows of a pitch that takes the byte loads, and a whole wave per row (more than 4096 int8 columns)
    run_case("tight", TIGHT, 40, 33, 3, 0, 37, big);
    run_case("tight-1135", TIGHT, 20, 1135, 2, 1, 30, big);
    run_case("whole-wave", INT8, 9, 5000, 3, 0, 9, big);
    run_case("whole-wave-packed", PACKED, 9, 16384, 2, 0, 9, big);
    // a row list with repeats; two slabs (the budget holds 64 rows of the groups), as a range and as a list
    run_case("list", INT8, 300, 130, 3, 1, 200, big);
    run_case("list-split", SPLIT, 90, 130, SNPM_SITE_MAX_GROUPS, 1, 129, big);
    run_case("two-slabs", PACKED, 120, 65, 3, 0, 100, 1);
    run_case("list-two-slabs", INT8, 50, 33, 2, 1, 128, 1);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
