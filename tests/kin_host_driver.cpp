// The kernel source of csrc/snpm_k_kin.hpp compiled for the host (tests/kin_host_shim/hip/hip_runtime.h stands in for the HIP
// header) and run with its launch geometry: every block by 256 real threads with a barrier for __syncthreads, the ballots of a wave
// through its 64 threads.  Built with -fsanitize=address,undefined by tests/test_kinship_cpu.py and run as a child process: the
// panel, the row and column lists, the planes and the results are heap blocks of exactly the size the library would use, the planes
// start with stale contents.  Every count is compared with a brute-force count.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <pthread.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"

using namespace snpm;

thread_local kin_dim3 threadIdx, blockIdx;
static pthread_barrier_t g_block_bar, g_wave_bar[KN_THREADS / WAVE];
static int g_pred[KN_THREADS / WAVE][2][WAVE];
static thread_local unsigned t_ballots;

void __syncthreads() { pthread_barrier_wait(&g_block_bar); }

// two buffers, one barrier per ballot: a thread that is already writing ballot n + 1 cannot disturb one still reading ballot n - 1,
// because every thread of the wave finished that read before it entered the barrier of ballot n
unsigned long long __ballot(int predicate)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, buf = t_ballots++ & 1;
    g_pred[wave][buf][lane] = predicate != 0;
    pthread_barrier_wait(&g_wave_bar[wave]);
    unsigned long long m = 0;
    for (int l = 0; l < WAVE; ++l) m |= (unsigned long long)g_pred[wave][buf][l] << l;
    return m;
}

struct Launch {
    unsigned gx, gy;
    std::function<void()> body;
};
static Launch g_launch;

static void *thread_main(void *arg)
{
    threadIdx = {(unsigned)(intptr_t)arg, 0, 0};
    for (unsigned by = 0; by < g_launch.gy; ++by)
        for (unsigned bx = 0; bx < g_launch.gx; ++bx) {
            blockIdx = {bx, by, 0};
            g_launch.body();
            pthread_barrier_wait(&g_block_bar);          // the next block reuses the `__shared__` statics
        }
    return nullptr;
}

static void launch(unsigned gx, unsigned gy, std::function<void()> body)
{
    g_launch = {gx, gy, body};
    pthread_t th[KN_THREADS];
    for (int t = 0; t < KN_THREADS; ++t)
        if (pthread_create(&th[t], nullptr, thread_main, (void *)(intptr_t)t)) { perror("pthread_create"); exit(3); }
    for (int t = 0; t < KN_THREADS; ++t) pthread_join(th[t], nullptr);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

enum Layout { INT8, PACKED, SPLIT };

// a panel of exactly the bytes its layout needs; calls[r * n_acc + a] keeps the values (-1 / 0 / 1 / 2, int8 panels also 3)
struct Panel {
    int8_t *d = nullptr;
    int64_t pitch = 0, desc = 0, n_snp = 0, n_acc = 0;
    std::vector<int8_t> calls;
};

static Panel make_panel(Layout lay, int64_t n_snp, int64_t n_acc)
{
    Panel p;
    p.n_snp = n_snp; p.n_acc = n_acc;
    p.calls.resize((size_t)(n_snp * n_acc));
    for (auto &c : p.calls) {
        const uint32_t u = rnd() % 100;
        c = (int8_t)(u < 12 ? -1 : u < 55 ? 0 : u < 90 ? 1 : (u < 97 || lay != INT8) ? 2 : 3);
    }
    for (int64_t r = 0; r < n_snp && n_acc > 2; ++r) p.calls[(size_t)(r * n_acc + 1)] = -1;       // an accession without a call
    size_t bytes;
    if (lay == INT8) {
        p.pitch = n_acc;
        bytes = (size_t)(n_snp * n_acc);
        p.d = (int8_t *)malloc(bytes ? bytes : 1);
        for (size_t i = 0; i < bytes; ++i) p.d[i] = p.calls[i] < 0 ? (int8_t)0xFF : p.calls[i];
        return p;
    }
    const int64_t row_bytes = (n_acc + 3) / 4;
    int64_t tail = 0, tail_off = 0;
    if (lay == SPLIT) {                     // main part: the whole 64-byte blocks of a row; tail: the rest, rows of 2^t bytes
        const int64_t main = row_bytes / 64 * 64, rem = row_bytes - main;
        tail = 4;
        while (tail < rem) tail <<= 1;
        p.pitch = main;
        tail_off = (n_snp * main + 255) / 256 * 256;
        int lg = 0;
        while (((int64_t)1 << lg) < tail) ++lg;
        p.desc = 1 | ((int64_t)(lg + 1) << 1) | ((tail_off / 256) << 8);
        bytes = (size_t)(tail_off + n_snp * tail);
    } else {
        p.pitch = row_bytes;
        p.desc = 1;
        bytes = (size_t)(n_snp * row_bytes);
    }
    p.d = (int8_t *)malloc(bytes ? bytes : 1);
    memset(p.d, 0xFF, bytes);
    for (int64_t r = 0; r < n_snp; ++r)
        for (int64_t b = 0; b < (lay == SPLIT ? p.pitch + tail : row_bytes); ++b) {
            unsigned out = 0;
            for (int f = 0; f < 4; ++f) {
                const int64_t a = 4 * b + f;
                const int v = a < n_acc ? p.calls[(size_t)(r * n_acc + a)] : -1;
                out |= (unsigned)(v < 0 ? 3 : v) << (2 * f);
            }
            ((uint8_t *)p.d)[pk_off(p.pitch, p.desc, r, b)] = (uint8_t)out;
        }
    return p;
}

static int g_fails = 0;

// what snpm_panel_kinship_counts does after its validation, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, int64_t n_rows, size_t ws_bytes)
{
    Panel p = make_panel(lay, n_snp, n_acc);
    int64_t ncols = n_acc, row0 = 0;
    int32_t *cols = nullptr;
    int64_t *rows = nullptr;
    if (use_cols) {                         // a shuffled subset with one repeat
        ncols = std::max<int64_t>(1, n_acc - n_acc / 3);
        cols = (int32_t *)malloc((size_t)ncols * sizeof(int32_t));
        for (int64_t a = 0; a < ncols; ++a) cols[a] = (int32_t)(rnd() % n_acc);
        if (ncols > 1) cols[ncols - 1] = cols[0];
    }
    if (use_rows) {                         // unsorted, with repeats
        rows = (int64_t *)malloc((size_t)std::max<int64_t>(1, n_rows) * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = (int64_t)(rnd() % n_snp);
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    const size_t cells = (size_t)(ncols * ncols);
    int32_t *out = (int32_t *)calloc(3 * cells, sizeof(int32_t));
    int32_t *o_ninfo = out, *o_same = out + cells, *o_diff = out + 2 * cells;
    int slabs = 0;
    if (n_rows > 0) {
        const int64_t cols_pad = (ncols + KN_PL_COLS - 1) / KN_PL_COLS * KN_PL_COLS;
        const int n_tiles = (int)((ncols + KN_TILE - 1) / KN_TILE);
        const int64_t step_rows = (int64_t)KN_STEP_WORDS * 64, steps_per_chunk = KN_CHUNK_WORDS / KN_STEP_WORDS;
        const int64_t step_bytes = 3 * cols_pad * KN_STEP_WORDS * 8;
        int64_t slab_steps = std::max<int64_t>(1, (int64_t)(ws_bytes / (size_t)step_bytes));
        if (slab_steps >= steps_per_chunk) slab_steps = slab_steps / steps_per_chunk * steps_per_chunk;
        slab_steps = std::min<int64_t>(slab_steps, (n_rows + step_rows - 1) / step_rows);
        const int64_t slab_rows = slab_steps * step_rows;
        const size_t plane_bytes = (size_t)(slab_steps * step_bytes);
        unsigned long long *planes = (unsigned long long *)malloc(plane_bytes);
        memset(planes, 0xA5, plane_bytes);                            // stale contents
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t W = (n_valid + step_rows - 1) / step_rows * KN_STEP_WORDS;
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab, as in the library
            const int64_t *slab_list = nullptr;
            if (rows) {
                int64_t *copy = (int64_t *)malloc((size_t)n_valid * sizeof(int64_t));
                memcpy(copy, rows + s0, (size_t)n_valid * sizeof(int64_t));
                slab_list = copy;
            }
            launch((unsigned)W, (unsigned)(cols_pad / KN_PL_COLS), [&] {
                k_kin_planes(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, (int)ncols, planes, cols_pad, W);
            });
            launch((unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + KN_CHUNK_WORDS - 1) / KN_CHUNK_WORDS), [&] {
                k_kin_count(planes, cols_pad, W, (int)ncols, n_tiles, o_ninfo, o_same, o_diff);
            });
            free((void *)slab_list);
        }
        free(planes);
    }
    // brute force
    long bad = 0;
    std::vector<int8_t> col_a((size_t)std::max<int64_t>(1, n_rows)), col_b((size_t)std::max<int64_t>(1, n_rows));
    for (int64_t a = 0; a < ncols; ++a) {
        const int64_t ca = cols ? cols[a] : a;
        for (int64_t r = 0; r < n_rows; ++r) col_a[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + ca)];
        for (int64_t b = a; b < ncols; ++b) {
            const int64_t cb = cols ? cols[b] : b;
            for (int64_t r = 0; r < n_rows; ++r) col_b[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + cb)];
            int32_t ni = 0, sa = 0, di = 0;
            for (int64_t r = 0; r < n_rows; ++r) {
                const int x = col_a[(size_t)r], y = col_b[(size_t)r];
                ni += x >= 0 && y >= 0;
                const bool hom = (x == 0 || x == 1) && (y == 0 || y == 1);
                sa += hom && x == y;
                di += hom && x != y;
            }
            for (int64_t at : {a * ncols + b, b * ncols + a})
                bad += o_ninfo[at] != ni || o_same[at] != sa || o_diff[at] != di;
        }
    }
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld slabs=%d %s\n", name, (int)lay, (long long)n_acc, (long long)ncols,
           (long long)n_rows, slabs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(out); free(rows); free(cols); free(p.d);
}

int main()
{
    pthread_barrier_init(&g_block_bar, nullptr, KN_THREADS);
    for (auto &b : g_wave_bar) pthread_barrier_init(&b, nullptr, WAVE);
    const size_t big = size_t(512) << 20;
    const int64_t chunk_rows = (int64_t)KN_CHUNK_WORDS * 64;
    int k = 0;
    for (int64_t acc : {1, 2, 31, 32, 33, 65, 130})
        for (int64_t rows : {0, 1, 63, 64, 65}) {
            const Layout lay = (Layout)(k++ % 3);
            run_case("small", lay, rows + 3, acc, 0, 0, rows, big);
        }
    run_case("chunk-1", INT8, chunk_rows + 5, 2, 0, 0, chunk_rows - 1, big);
    run_case("chunk", PACKED, chunk_rows + 5, 33, 0, 0, chunk_rows, big);
    run_case("chunk+1", SPLIT, chunk_rows + 5, 2, 0, 0, chunk_rows + 1, big);
    // two slabs: one chunk per slab (the budget holds one chunk of the 64 padded columns), and slabs below a chunk (one LDS step each)
    run_case("two-slabs", INT8, chunk_rows + 1100, 33, 0, 0, chunk_rows + 1030, (size_t)(3 * 64 * KN_CHUNK_WORDS * 8));
    run_case("two-short-slabs", PACKED, 1100, 65, 0, 0, 1030, 1);
    // column and row lists; the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28)
    run_case("lists", INT8, 300, 70, 1, 1, 200, big);
    run_case("lists-packed", SPLIT, 90, 130, 1, 1, 129, big);
    run_case("list-two-slabs", INT8, 500, 33, 1, 1, 2100, 1);
    run_case("split-wide", SPLIT, 65, 1135, 0, 0, 65, big);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
