// The kernel source of csrc/snpm_k_pca.hpp (and k_win_planes of csrc/snpm_k_win.hpp, which k_pca_gram is launched behind) compiled
// for the host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header, tests/host_kernel/harness.hpp runs it) with its
// launch geometry: every block by 256 real threads with a barrier for __syncthreads, the ballots and exchanges of a wave through its
// 64 threads.  Built with -fsanitize=address,undefined by tests/test_pca_cpu.py and run as a child process: the panel, the row and
// column lists, the table rows of a slab, the planes, the partials, the padded vec and the results are heap blocks of exactly the size
// the library would use, the pad bytes of the rows hold arbitrary values and the workspaces start with stale contents; the slab plans
// are the library's own (pca_slab_steps, pca_gram_splits, pca_load_slab_rows).  Tables and vectors hold small integers, so every sum
// is exact whatever its order and is compared with a plain loop without a tolerance.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"
#include "snpm_k_pca.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;

enum Fill { RANDOM, ALL_MISSING, WITH_CODE3 };

// the launches of snpm_panel_gram and snpm_panel_loadings, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, int64_t row0, int64_t n_rows, int k,
                     size_t ws_bytes, Fill fill = RANDOM)
{
    Panel p = make_panel(lay, n_snp, n_acc, kStyle);
    if (fill != RANDOM) {                   // rewrite the calls: every call missing, or every fifth call of an int8 panel the "other" code
        for (int64_t r = 0; r < n_snp; ++r)
            for (int64_t a = 0; a < n_acc; ++a) {
                int8_t &c = p.calls[(size_t)(r * n_acc + a)];
                c = fill == ALL_MISSING ? (int8_t)-1 : (int8_t)((r + a) % 5 == 0 ? 3 : c);
                if (!p.packed) p.d[r * p.pitch + a] = c >= 0 ? c : (int8_t)(0x80 | (rnd() & 0x7F));
            }
        if (p.packed) {
            for (int64_t r = 0; r < n_snp; ++r)
                for (int64_t b = 0; b < (n_acc + 3) / 4; ++b) ((uint8_t *)p.d)[pk_off(p.pitch, p.desc, r, b)] = 0xFF;
        }
    }
    int64_t ncols = n_acc;
    int32_t *cols = nullptr;
    int64_t *rows = nullptr;
    if (use_cols) {                         // descending, with a repeat
        ncols = std::max<int64_t>(1, n_acc - n_acc / 3);
        cols = (int32_t *)exact_block((size_t)ncols * sizeof(int32_t));
        for (int64_t a = 0; a < ncols; ++a) cols[a] = (int32_t)(n_acc - 1 - a);
        if (ncols > 1) cols[ncols - 1] = cols[0];
    }
    if (use_rows) {                         // unsorted, with repeats
        rows = (int64_t *)exact_block((size_t)n_rows * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = (int64_t)(rnd() % n_snp);
        if (n_rows > 1) rows[n_rows - 1] = rows[0];
    }
    double *tab = (double *)exact_block((size_t)n_rows * 4 * sizeof(double));
    for (int64_t i = 0; i < n_rows * 4; ++i) tab[i] = (double)((int)(rnd() % 7) - 3);
    if (fill == WITH_CODE3)
        for (int64_t r = 0; r < n_rows; ++r) tab[4 * r + 3] = 2.0;
    double *vec = (double *)exact_block((size_t)(ncols * k) * sizeof(double));
    for (int64_t i = 0; i < ncols * k; ++i) vec[i] = (double)((int)(rnd() % 9) - 4);
    const size_t cells = (size_t)(ncols * ncols);
    double *gram = (double *)calloc(cells, sizeof(double));          // (the library zeroes the device matrix before the first slab)
    double *load = (double *)exact_block((size_t)(n_rows * k) * sizeof(double));
    memset(load, 0xA5, (size_t)(n_rows * k) * sizeof(double));
    int slabs = 0, splits = 0;
    {   // ---- snpm_panel_gram
        const int64_t cols_pad = (ncols + PCA_PL_COLS - 1) / PCA_PL_COLS * PCA_PL_COLS;
        const int n_tiles = (int)(cols_pad / PCA_TILE), n_pairs = n_tiles * (n_tiles + 1) / 2;
        splits = pca_gram_splits(n_pairs);
        const int64_t slab_steps = pca_slab_steps(ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * PCA_STEP_ROWS;
        const size_t plane_bytes = (size_t)(slab_steps * 4 * cols_pad * PCA_STEP_WORDS * 8);
        const size_t part_bytes = (size_t)splits * (size_t)n_pairs * PCA_TILE * PCA_TILE * sizeof(double);
        unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
        double *part = (double *)exact_block(part_bytes);
        memset(planes, 0xA5, plane_bytes);                           // stale contents
        memset(part, 0x5A, part_bytes);
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t W = (n_valid + PCA_STEP_ROWS - 1) / PCA_STEP_ROWS * PCA_STEP_WORDS;
            const int64_t first = rows ? 0 : row0 + s0;              // a row list and the table travel slab by slab, as in the library
            int64_t *slab_list = nullptr;
            if (rows) {
                slab_list = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(slab_list, rows + s0, (size_t)n_valid * sizeof(int64_t));
            }
            double *slab_tab = (double *)exact_block((size_t)n_valid * 4 * sizeof(double));
            memcpy(slab_tab, tab + 4 * s0, (size_t)n_valid * 4 * sizeof(double));
            launch(WN_THREADS, (unsigned)W, (unsigned)(cols_pad / PCA_PL_COLS), [&] {
                k_win_planes(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, ncols, planes, cols_pad, W);
            });
            launch(PCA_THREADS, (unsigned)n_pairs, (unsigned)splits, [&] { k_pca_gram(planes, cols_pad, W, slab_tab, n_valid, n_tiles, part); });
            launch(PCA_THREADS, (unsigned)((cells + PCA_THREADS - 1) / PCA_THREADS), 1, [&] { k_pca_fold(part, n_tiles, n_pairs, splits, ncols, gram); });
            free(slab_tab);
            free(slab_list);
        }
        free(part);
        free(planes);
    }
    int load_slabs = 0;
    {   // ---- snpm_panel_loadings
        const int kp = pca_load_pitch(k);
        double *vecp = (double *)exact_block((size_t)(ncols * kp) * sizeof(double));
        memset(vecp, 0, (size_t)(ncols * kp) * sizeof(double));
        for (int64_t a = 0; a < ncols; ++a) memcpy(vecp + a * kp, vec + a * k, (size_t)k * sizeof(double));
        const int64_t slab_rows = pca_load_slab_rows(ws_bytes, k, n_rows);
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++load_slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t first = rows ? 0 : row0 + s0;
            int64_t *slab_list = nullptr;
            if (rows) {
                slab_list = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(slab_list, rows + s0, (size_t)n_valid * sizeof(int64_t));
            }
            double *slab_tab = (double *)exact_block((size_t)n_valid * 4 * sizeof(double));
            memcpy(slab_tab, tab + 4 * s0, (size_t)n_valid * 4 * sizeof(double));
            double *slab_load = (double *)exact_block((size_t)(n_valid * k) * sizeof(double));
            memset(slab_load, 0x5A, (size_t)(n_valid * k) * sizeof(double));
            constexpr int waves = PCA_LOAD_THREADS / WAVE;
            const int64_t blocks = std::min<int64_t>((n_valid + waves - 1) / waves, 3);      // (any number: the waves stride the rows)
            launch(PCA_LOAD_THREADS, (unsigned)blocks, 1, [&] {
                k_pca_load(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, ncols, slab_tab, vecp, k, slab_load);
            });
            memcpy(load + s0 * k, slab_load, (size_t)(n_valid * k) * sizeof(double));
            free(slab_load);
            free(slab_tab);
            free(slab_list);
        }
        free(vecp);
    }
    // the plain loops
    long bad = 0;
    std::vector<double> t((size_t)(n_rows * ncols));
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t a = 0; a < ncols; ++a) {
            const int8_t c = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + (cols ? cols[a] : a))];
            t[(size_t)(r * ncols + a)] = c < 0 ? 0.0 : tab[4 * r + c];
        }
    for (int64_t a = 0; a < ncols; ++a)
        for (int64_t b = 0; b < ncols; ++b) {
            double s = 0.0;
            for (int64_t r = 0; r < n_rows; ++r) s += t[(size_t)(r * ncols + a)] * t[(size_t)(r * ncols + b)];
            bad += gram[a * ncols + b] != s;
        }
    for (int64_t r = 0; r < n_rows; ++r)
        for (int c = 0; c < k; ++c) {
            double s = 0.0;
            for (int64_t a = 0; a < ncols; ++a) s += t[(size_t)(r * ncols + a)] * vec[a * k + c];
            bad += load[r * k + c] != s;
        }
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld k=%d splits=%d slabs=%d load_slabs=%d %s\n", name, (int)lay, (long long)n_acc, (long long)ncols,
           (long long)n_rows, k, splits, slabs, load_slabs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(load); free(gram); free(vec); free(tab); free(rows); free(cols); free(p.d);
}

static void plan_case(const char *name, int64_t got, int64_t want)
{
    printf("case %s got=%lld want=%lld %s\n", name, (long long)got, (long long)want, got == want ? "ok" : "MISMATCH");
    g_fails += got != want;
}

int main()
{
    const size_t big = size_t(512) << 20;
    const int ks[4] = {1, 2, 10, 32};
    int n = 0;
    // every width around a tile of 64 with two of the row counts around a word, a pass, a plane step and beyond, in turn
    const int64_t row_counts[8] = {1, 63, 64, 65, 1023, 1024, 1025, 2500};
    for (int64_t acc : {1, 2, 31, 32, 33, 63, 64, 65, 129, 130})
        for (int pick = 0; pick < 2; ++pick) {
            const int64_t rows = row_counts[n % 8];      // (n counts the cases: every row count comes up at least twice)
            const Layout lay = (Layout)(n % 3);
            run_case("grid", lay, rows + 3, acc, 0, 0, 0, rows, ks[n % 4], big);
            ++n;
        }
    // column lists in descending order with a repeat, row lists unsorted with repeats; a dense range that does not start at row 0
    run_case("lists", INT8, 300, 70, 1, 1, 0, 200, 10, big);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, 0, 129, 2, big);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, 0, 129, 32, big);
    run_case("row0", INT8, 200, 33, 0, 0, 57, 143, 2, big);
    run_case("all-missing", PACKED, 70, 33, 0, 0, 0, 70, 1, big, ALL_MISSING);
    run_case("code3", INT8, 130, 65, 0, 0, 0, 130, 10, big, WITH_CODE3);
    // three slabs, the last one partial: a budget below one step takes one step of 1024 rows per slab (and 64 rows per slab of loadings)
    run_case("three-slabs", INT8, 2200, 33, 0, 0, 0, 2100, 2, 1);
    run_case("list-three-slabs", SPLIT, 500, 65, 1, 1, 0, 2100, 10, 1);
    // the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28)
    run_case("split-wide", SPLIT, 40, 1135, 0, 0, 0, 40, 32, big);
    // the plans alone
    plan_case("plan-one-step", pca_slab_steps(1, 64, INT32_MAX), 1);
    plan_case("plan-fit", pca_slab_steps((size_t)(3 * pca_step_bytes(1152) + 5), 1152, INT32_MAX), 3);
    plan_case("plan-need", pca_slab_steps(big, 64, 1025), 2);
    plan_case("plan-splits", pca_gram_splits(1) * 1000000 + pca_gram_splits(171) * 1000 + pca_gram_splits(16471), 32 * 1000000 + 3 * 1000 + 1);
    plan_case("plan-load-rows", pca_load_slab_rows(1, 32, 1000) * 1000000 + pca_load_slab_rows(big, 1, 1000), 64 * 1000000 + 1000);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
