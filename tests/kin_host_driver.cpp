// The kernel source of csrc/snpm_k_kin.hpp compiled for the host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header,
// tests/host_kernel/harness.hpp runs it) with its launch geometry: every block by 256 real threads with a barrier for __syncthreads,
// the ballots of a wave through its 64 threads.  Built with -fsanitize=address,undefined by tests/test_kinship_cpu.py and run as a
// child process: the panel, the row and column lists, the planes and the results are heap blocks of exactly the size the library
// would use, the planes start with stale contents; the slab plan is the library's own (kin_slab_steps).  Every count is compared
// with a brute-force count.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"

#include "harness.hpp"

// rows of exactly their bytes, 0xFF in every pad byte, an accession without a call
static const PanelStyle kStyle = {false, false, true};

static int g_fails = 0;

// the launches of snpm_panel_kinship_counts, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, int64_t n_rows, size_t ws_bytes)
{
    Panel p = make_panel(lay, n_snp, n_acc, kStyle);
    int64_t ncols = n_acc, row0 = 0;
    int32_t *cols = nullptr;
    int64_t *rows = nullptr;
    if (use_cols) {                         // a shuffled subset with one repeat
        ncols = std::max<int64_t>(1, n_acc - n_acc / 3);
        cols = (int32_t *)exact_block((size_t)ncols * sizeof(int32_t));
        for (int64_t a = 0; a < ncols; ++a) cols[a] = (int32_t)(rnd() % n_acc);
        if (ncols > 1) cols[ncols - 1] = cols[0];
    }
    if (use_rows) {                         // unsorted, with repeats
        rows = (int64_t *)exact_block((size_t)n_rows * sizeof(int64_t));
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
        const int64_t slab_steps = kin_slab_steps(ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * KN_STEP_ROWS;
        const size_t plane_bytes = (size_t)(slab_steps * kin_step_bytes(cols_pad));
        unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
        memset(planes, 0xA5, plane_bytes);                            // stale contents
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t W = (n_valid + KN_STEP_ROWS - 1) / KN_STEP_ROWS * KN_STEP_WORDS;
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab, as in the library
            const int64_t *slab_list = nullptr;
            if (rows) {
                int64_t *copy = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(copy, rows + s0, (size_t)n_valid * sizeof(int64_t));
                slab_list = copy;
            }
            launch(KN_THREADS, (unsigned)W, (unsigned)(cols_pad / KN_PL_COLS), [&] {
                k_kin_planes(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, (int)ncols, planes, cols_pad, W);
            });
            launch(KN_THREADS, (unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + KN_CHUNK_WORDS - 1) / KN_CHUNK_WORDS), [&] {
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

static void plan_case(const char *name, int64_t steps, int64_t want)
{
    printf("case %s steps=%lld want=%lld %s\n", name, (long long)steps, (long long)want, steps == want ? "ok" : "MISMATCH");
    g_fails += steps != want;
}

int main()
{
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
    // the plan alone: 65535 chunks (grid.y of k_kin_count) of 8 steps bound a slab however large the budget; a budget below one step takes one
    plan_case("plan-grid-cap", kin_slab_steps(SIZE_MAX, 64, INT32_MAX), 65535 * (KN_CHUNK_WORDS / KN_STEP_WORDS));
    plan_case("plan-one-step", kin_slab_steps(1, 64, INT32_MAX), 1);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
