// The kernel source of csrc/snpm_k_sim.hpp (and k_win_planes of csrc/snpm_k_win.hpp, which it is launched behind) compiled for the
// host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header, tests/host_kernel/harness.hpp runs it) with its launch
// geometry: every block by 256 real threads with a barrier for __syncthreads, the ballots of a wave through its 64 threads.  Built
// with -fsanitize=address,undefined by tests/test_power_cpu.py and run as a child process: the panel, the row and column lists, the
// group offsets, the seven planes and the results are heap blocks of exactly the size the library would use, the pad bytes of the
// rows hold arbitrary values and the planes start with stale contents; the slab plan is the library's own (sim_slab_steps).  Every
// count is compared with a brute-force count.  A case of more than 2100 rows takes its four DB planes from the host (planes_on_host: the
// layout k_win_planes writes, over the stale block) unless it says otherwise -- a block of that unchanged kernel costs 64 exchanges
// among 64 threads here, and tests/win_host_driver.cpp covers it; the kernels of this family run in every case.  Prints "case ... ok"
// per case, the hash table ("case hash ...") that the test compares with the numpy twin, and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"
#include "snpm_k_f1x.hpp"
#include "snpm_k_sim.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;

static const unsigned long long kFull = 1ull << 32;     // err_thr of error rate 1
static unsigned long long thr_of(double rate) { return (unsigned long long)(rate * 4294967296.0); }

// what k_win_planes writes for a slab, every word of [4][cols_pad][W]
static void planes_on_host(const Panel &p, const int64_t *rows, int64_t first, int64_t n_valid, const int32_t *cols, int64_t ncols,
                           unsigned long long *planes, int64_t cols_pad, int64_t W)
{
    memset(planes, 0, (size_t)(4 * cols_pad * W) * sizeof(unsigned long long));
    for (int64_t k = 0; k < n_valid; ++k) {
        const int64_t prow = rows ? rows[first + k] : first + k;
        for (int64_t a = 0; a < ncols; ++a) {
            const int c = p.calls[(size_t)(prow * p.n_acc + (cols ? cols[a] : a))];
            if (c < 0) continue;
            const unsigned long long bit = 1ull << (k & 63);
            if (c <= 2) planes[c * cols_pad * W + a * W + (k >> 6)] |= bit;
            planes[3 * cols_pad * W + a * W + (k >> 6)] |= bit;
        }
    }
}

// the launches of snpm_panel_sim_counts, with `ws_bytes` as the workspace budget.  `bounds`: the inner group boundaries
// (grp_off[1 .. n_grp - 1]); 0 and n_rows are added here.
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, int64_t n_rows,
                     std::vector<int64_t> bounds, unsigned long long err_thr, unsigned long long seed, size_t ws_bytes, bool device_planes = false)
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
    const int n_grp = (int)bounds.size() + 1;
    int64_t *grp_off = (int64_t *)exact_block((size_t)(n_grp + 1) * sizeof(int64_t));
    grp_off[0] = 0;
    for (int g = 1; g < n_grp; ++g) grp_off[g] = std::min(bounds[(size_t)(g - 1)], n_rows);
    grp_off[n_grp] = n_rows;
    const size_t cells = (size_t)(n_grp * ncols * ncols);
    int32_t *out = (int32_t *)exact_block(2 * cells * sizeof(int32_t));
    memset(out, 0, 2 * cells * sizeof(int32_t));
    int32_t *o_score = out, *o_ninfo = out + cells;
    int slabs = 0;
    if (n_rows > 0) {
        const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
        const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
        const int64_t slab_steps = sim_slab_steps(ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * F1X_STEP_ROWS;
        const size_t plane_bytes = (size_t)(slab_steps * sim_step_bytes(cols_pad));
        const size_t slab_plane_words = (size_t)(cols_pad * slab_steps * F1X_STEP_WORDS);
        unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
        memset(planes, 0xA5, plane_bytes);                            // stale contents
        unsigned long long *q = planes + F1X_PLANES * slab_plane_words;
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
            if (n_rows <= 2100 || device_planes)
                launch(WN_THREADS, (unsigned)W, (unsigned)(cols_pad / F1X_PL_COLS), [&] {
                    k_win_planes(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, ncols, planes, cols_pad, W);
                });
            else
                planes_on_host(p, slab_list, first, n_valid, cols, ncols, planes, cols_pad, W);
            if (err_thr)
                launch(SIM_THREADS, (unsigned)((W + WAVE - 1) / WAVE), (unsigned)(cols_pad / (SIM_THREADS / WAVE)), [&] {
                    k_sim_noise(planes, q, cols_pad, W, s0, err_thr, seed);
                });
            launch(SIM_THREADS, (unsigned)(n_tiles * n_tiles), (unsigned)((W + F1X_CHUNK_WORDS - 1) / F1X_CHUNK_WORDS), [&] {
                k_sim_count(planes, err_thr ? q : planes, cols_pad, W, s0, grp_off, n_grp, (int)ncols, n_tiles, o_score, o_ninfo);
            });
            free((void *)slab_list);
        }
        free(planes);
    }
    // brute force, row by row
    std::vector<int32_t> w_score(cells, 0), w_ninfo(cells, 0);
    std::vector<int> code((size_t)ncols);
    long changed = 0;
    for (int g = 0; g < n_grp; ++g)
        for (int64_t k = grp_off[g]; k < grp_off[g + 1]; ++k) {
            const int64_t prow = rows ? rows[k] : row0 + k;
            for (int64_t a = 0; a < ncols; ++a) code[(size_t)a] = p.calls[(size_t)(prow * n_acc + (cols ? cols[a] : a))];
            for (int64_t a = 0; a < ncols; ++a) {
                int c = code[(size_t)a];
                if (c < 0 || c > 2) continue;
                const uint64_t h = sim_hash(seed, (uint64_t)a, (uint64_t)k);
                if ((h >> 32) < err_thr) {
                    const int d = (int)(((h & 0xFFFFFFFFull) * 3ull) >> 32);
                    changed += d != c;
                    c = d;
                }
                int32_t *ws = w_score.data() + ((size_t)g * ncols + a) * ncols, *wn = w_ninfo.data() + ((size_t)g * ncols + a) * ncols;
                for (int64_t b = 0; b < ncols; ++b) {
                    wn[b] += code[(size_t)b] >= 0;
                    ws[b] += code[(size_t)b] == c;
                }
            }
        }
    long bad = 0;
    for (size_t at = 0; at < cells; ++at) bad += o_score[at] != w_score[at] || o_ninfo[at] != w_ninfo[at];
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld groups=%d thr=%llu changed=%ld slabs=%d %s\n", name, (int)lay, (long long)n_acc,
           (long long)ncols, (long long)n_rows, n_grp, err_thr, changed, slabs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(out); free(grp_off); free(rows); free(cols); free(p.d);
}

static void plan_case(const char *name, int64_t steps, int64_t want)
{
    printf("case %s steps=%lld want=%lld %s\n", name, (long long)steps, (long long)want, steps == want ? "ok" : "MISMATCH");
    g_fails += steps != want;
}

int main()
{
    const size_t big = size_t(512) << 20;
    const unsigned long long p05 = thr_of(0.05), half = thr_of(0.5);
    // the hash, for the numpy twin to agree with
    for (unsigned long long seed : {0ull, 1ull, 0xFFFFFFFFFFFFFFFFull, 0x123456789ABCDEFull})
        for (unsigned long long a : {0ull, 1ull, 11551ull})
            for (unsigned long long k : {0ull, 1ull, 63ull, 64ull, 0x7FFFFFFFull, 0x100000000ull, 0xFEDCBA9876543210ull})
                printf("case hash seed=%llu a=%llu k=%llu h=%llu ok\n", seed, a, k, (unsigned long long)sim_hash(seed, a, k));
    // accessions x rows: the tile sides of the count kernel (32) and of the plane kernel (64), words, LDS steps, chunks
    int k = 0;
    for (int64_t acc : {1, 2, 31, 32, 33, 65, 130})
        for (int64_t rows : {0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193}) {
            const Layout lay = (Layout)(k % 3);
            const unsigned long long thr = (k % 4 == 0) ? 0ull : (k % 4 == 1) ? p05 : (k % 4 == 2) ? half : kFull;
            std::vector<int64_t> bounds;
            if (k % 2) bounds = {rows / 3, rows / 3, rows - rows / 5};
            ++k;
            run_case("shape", lay, rows + 3, acc, 0, 0, rows, bounds, thr, 1000 + (unsigned long long)k, big);
        }
    // group boundaries, in every layout
    for (Layout lay : {INT8, PACKED, SPLIT}) {
        run_case("one-group", lay, 8200, 33, 0, 0, 8200, {}, p05, 7, big);
        run_case("bounds", lay, 8200, 33, 0, 0, 8200, {1, 63, 64, 65, 1024, 8192, 8193}, p05, 7, big);
        run_case("three-in-a-word", lay, 210, 65, 0, 0, 200, {70, 75, 100}, half, 8, big);
        run_case("empty-groups", lay, 1500, 33, 0, 0, 1400, {0, 0, 500, 500, 500, 1100, 1400, 1400}, p05, 9, big);
    }
    {
        std::vector<int64_t> b63;
        for (int g = 1; g < 64; ++g) b63.push_back((int64_t)g * g);      // 1, 4, 9, ... 3969: many in the first words, then words apart
        run_case("64-groups", INT8, 4100, 33, 0, 0, 4000, b63, p05, 10, big);
        run_case("64-groups", SPLIT, 4100, 2, 0, 0, 4000, b63, kFull, 10, big);
    }
    // error rates on one shape
    for (unsigned long long thr : {0ull, p05, half, kFull}) run_case("rates", PACKED, 1100, 33, 0, 0, 1030, {500}, thr, 11, big);
    // column lists with a repeat, unsorted row lists with repeats
    run_case("lists", INT8, 300, 70, 1, 1, 200, {64}, half, 12, big);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, 129, {}, 0, 12, big);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, 129, {100}, p05, 12, big);
    // slabs: three of one LDS step each, groups across the slab edges; one chunk per slab
    run_case("three-short-slabs", SPLIT, 2200, 33, 0, 0, 2100, {1000, 1024, 2050}, half, 13, 1);
    run_case("list-three-slabs", INT8, 500, 33, 1, 1, 2100, {1030}, p05, 13, 1);
    run_case("two-slabs", PACKED, 8192 + 1100, 33, 0, 0, 8192 + 1030, {8192}, p05, 13, (size_t)(7 * 64 * F1X_CHUNK_WORDS * 8), true);
    // the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28)
    run_case("split-wide", SPLIT, 2048, 1135, 0, 0, 2048, {100, 1030}, p05, 14, big);
    run_case("split-wide-planes", SPLIT, 135, 1135, 0, 0, 130, {100}, p05, 14, big);
    // the plan alone: 65535 chunks (grid.y of k_sim_count) of 8 steps bound a slab however large the budget; a budget below one step takes one
    plan_case("plan-grid-cap", sim_slab_steps(SIZE_MAX, 64, INT32_MAX), 65535 * (F1X_CHUNK_WORDS / F1X_STEP_WORDS));
    plan_case("plan-one-step", sim_slab_steps(1, 64, INT32_MAX), 1);
    plan_case("plan-seven-planes", sim_slab_steps((size_t)(7 * 64 * F1X_STEP_WORDS * 8) * 3 - 1, 64, INT32_MAX), 2);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
