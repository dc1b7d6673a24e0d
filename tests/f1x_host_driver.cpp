// The kernel source of csrc/snpm_k_f1x.hpp (and k_win_planes of csrc/snpm_k_win.hpp, which it is launched behind) compiled for the
// host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header, tests/host_kernel/harness.hpp runs it) with its launch
// geometry: every block by 256 real threads with a barrier for __syncthreads, the ballots of a wave through its 64 threads.  Built
// with -fsanitize=address,undefined by tests/test_f1search_cpu.py and run as a child process: the panel, the row and column lists,
// the classes, the masks, the planes and the results are heap blocks of exactly the size the library would use, the pad bytes of the
// rows hold arbitrary values and the planes start with stale contents; the slab plan and the masks are the library's own
// (f1x_slab_steps, f1x_fill_masks).  Every count is compared with a brute-force count.  Prints "case ... ok" per case and
// "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"
#include "snpm_k_f1x.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;

// the launches of snpm_panel_f1_counts, with `ws_bytes` as the workspace budget
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
        if (n_rows > 1) rows[n_rows - 1] = rows[0];
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    uint8_t *cls = (uint8_t *)exact_block((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) {
        const uint32_t u = rnd() % 100;
        cls[r] = (uint8_t)(u < 40 ? 0 : u < 70 ? 1 : u < 92 ? 2 : 0xFF);
    }
    const size_t cells = (size_t)(ncols * ncols);
    int32_t *out = (int32_t *)calloc(2 * cells, sizeof(int32_t));
    int32_t *o_hits = out, *o_ninfo = out + cells;
    int slabs = 0;
    {
        const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
        const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
        const int64_t slab_steps = f1x_slab_steps(ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * F1X_STEP_ROWS;
        const size_t plane_bytes = (size_t)(slab_steps * f1x_step_bytes(cols_pad));
        unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
        memset(planes, 0xA5, plane_bytes);                            // stale contents
        const int64_t all_steps = (n_rows + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS;
        unsigned long long *masks = (unsigned long long *)exact_block((size_t)(all_steps * F1X_MASK_WORDS) * sizeof(unsigned long long));
        memset(masks, 0x5A, (size_t)(all_steps * F1X_MASK_WORDS) * sizeof(unsigned long long));
        f1x_fill_masks(cls, n_rows, masks);
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t W = (n_valid + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS * F1X_STEP_WORDS;
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab, as in the library
            const int64_t *slab_list = nullptr;
            if (rows) {
                int64_t *copy = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(copy, rows + s0, (size_t)n_valid * sizeof(int64_t));
                slab_list = copy;
            }
            launch(WN_THREADS, (unsigned)W, (unsigned)(cols_pad / F1X_PL_COLS), [&] {
                k_win_planes(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, ncols, planes, cols_pad, W);
            });
            const unsigned long long *slab_masks = masks + s0 / F1X_STEP_ROWS * F1X_MASK_WORDS;
            launch(F1X_THREADS, (unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + F1X_CHUNK_WORDS - 1) / F1X_CHUNK_WORDS), [&] {
                k_f1x_count(planes, cols_pad, W, slab_masks, (int)ncols, n_tiles, o_hits, o_ninfo);
            });
            free((void *)slab_list);
        }
        free(masks);
        free(planes);
    }
    // brute force
    long bad = 0, none = 0;
    std::vector<int8_t> col_a((size_t)n_rows), col_b((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) none += cls[r] == 0xFF;
    for (int64_t a = 0; a < ncols; ++a) {
        const int64_t ca = cols ? cols[a] : a;
        for (int64_t r = 0; r < n_rows; ++r) col_a[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + ca)];
        for (int64_t b = a; b < ncols; ++b) {
            const int64_t cb = cols ? cols[b] : b;
            for (int64_t r = 0; r < n_rows; ++r) col_b[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + cb)];
            int32_t ni = 0, hi = 0;
            for (int64_t r = 0; r < n_rows; ++r) {
                const int x = col_a[(size_t)r], y = col_b[(size_t)r];
                const int f1 = (x == 0 && y == 0) ? 0 : (x == 1 && y == 1) ? 1 : (x >= 0 && y >= 0 && x != y) ? 2 : -1;
                ni += f1 >= 0;
                hi += f1 >= 0 && f1 == (int)cls[r];
            }
            for (int64_t at : {a * ncols + b, b * ncols + a})
                bad += o_ninfo[at] != ni || o_hits[at] != hi;
        }
    }
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld noclass=%ld slabs=%d %s\n", name, (int)lay, (long long)n_acc, (long long)ncols,
           (long long)n_rows, none, slabs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(out); free(cls); free(rows); free(cols); free(p.d);
}

static void plan_case(const char *name, int64_t steps, int64_t want)
{
    printf("case %s steps=%lld want=%lld %s\n", name, (long long)steps, (long long)want, steps == want ? "ok" : "MISMATCH");
    g_fails += steps != want;
}

int main()
{
    const size_t big = size_t(512) << 20;
    const int64_t chunk_rows = (int64_t)F1X_CHUNK_WORDS * 64, step_rows = F1X_STEP_ROWS;
    int k = 0;
    for (int64_t acc : {1, 2, 31, 32, 33, 65, 130})
        for (int64_t rows : {1, 63, 64, 65}) {
            const Layout lay = (Layout)(k++ % 3);
            run_case("small", lay, rows + 3, acc, 0, 0, rows, big);
        }
    // one row past an LDS step and past a chunk, in every layout
    run_case("step+1", INT8, step_rows + 5, 33, 0, 0, step_rows + 1, big);
    run_case("step+1", PACKED, step_rows + 5, 65, 0, 0, step_rows + 1, big);
    run_case("step+1", SPLIT, step_rows + 5, 2, 0, 0, step_rows + 1, big);
    run_case("chunk+1", INT8, chunk_rows + 5, 2, 0, 0, chunk_rows + 1, big);
    run_case("chunk+1", PACKED, chunk_rows + 5, 33, 0, 0, chunk_rows + 1, big);
    run_case("chunk+1", SPLIT, chunk_rows + 5, 33, 0, 0, chunk_rows + 1, big);
    // two slabs: one chunk per slab (the budget holds one chunk of the 64 padded columns), and slabs below a chunk (one LDS step each)
    run_case("two-slabs", INT8, chunk_rows + 1100, 33, 0, 0, chunk_rows + 1030, (size_t)(4 * 64 * F1X_CHUNK_WORDS * 8));
    run_case("two-short-slabs", PACKED, 1100, 65, 0, 0, 1030, 1);
    run_case("three-short-slabs", SPLIT, 2200, 33, 0, 0, 2100, 1);
    // column and row lists; the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28)
    run_case("lists", INT8, 300, 70, 1, 1, 200, big);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, 129, big);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, 129, big);
    run_case("list-three-slabs", INT8, 500, 33, 1, 1, 2100, 1);
    run_case("split-wide", SPLIT, 65, 1135, 0, 0, 65, big);
    // the plan alone: 65535 chunks (grid.y of k_f1x_count) of 8 steps bound a slab however large the budget; a budget below one step takes one
    plan_case("plan-grid-cap", f1x_slab_steps(SIZE_MAX, 64, INT32_MAX), 65535 * (F1X_CHUNK_WORDS / F1X_STEP_WORDS));
    plan_case("plan-one-step", f1x_slab_steps(1, 64, INT32_MAX), 1);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
