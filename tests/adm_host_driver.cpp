// The kernel source of csrc/snpm_k_adm.hpp compiled for the host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header,
// tests/host_kernel/harness.hpp runs it) with its launch geometry: every block by its real threads (256, and 1024 for k_adm_fold) with
// a barrier for __syncthreads, the exchanges of a wave through its 64 threads.  Built with -fsanitize=address,undefined by
// tests/test_admixture_cpu.py and run as a child process: the panel, the row and column lists, both copies of Q and F in rows of
// adm_pitch(K) doubles, the partials, the two buffers of the likelihood tree and the result are heap blocks of exactly the size the
// library would use, the pad bytes of the panel rows hold arbitrary values and the workspaces start with stale contents; the plans are
// the library's own (adm_pitch, adm_split_rows, adm_splits, adm_ll_blocks).  One iteration is compared with a plain loop in long double
// (64-bit mantissa) within the bounds of the issue: every entry of F' within (ncols + 64) 2^-52 relative, of Q' within (n_rows + 64)
// 2^-52 relative, |ll - ref| <= 2^-52 ((K + 2) cells + (ceil(ncols / 64) + 64) |ref|).  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_pca.hpp"
#include "snpm_k_adm.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;

enum Fill { RANDOM, ALL_MISSING, WITH_CODE3, BLANK_ROWS_AND_COLUMNS };
constexpr unsigned UPDATE_F = 1u, UPDATE_Q = 2u;

static double unit() { return (rnd() + 0.5) / 4294967296.0; }

template <int KT>
static void launch_iteration(const Panel &p, const int64_t *rows, int64_t first, int64_t n_rows, const int32_t *cols, int64_t ncols, int K, unsigned flags,
                             const double *q_old, double *q_new, const double *f_old, double *f_new, double *part, double *ll_a, double *ll_b, double *out)
{
    const int64_t n_ll = adm_ll_blocks(n_rows), splits = adm_splits(n_rows, ncols);
    launch(ADM_ROWS_THREADS, (unsigned)n_ll, 1, [&] {
        k_adm_rows<KT>(p.d, p.pitch, p.desc, rows, first, n_rows, cols, ncols, q_old, f_old, K, (int)(flags & UPDATE_F), f_new, ll_a);
    });
    if (flags & UPDATE_Q)
        launch(ADM_COLS_THREADS, (unsigned)((ncols + ADM_COLS_THREADS - 1) / ADM_COLS_THREADS), (unsigned)splits, [&] {
            k_adm_cols<KT>(p.d, p.pitch, p.desc, rows, first, n_rows, adm_split_rows(n_rows, ncols), cols, ncols, q_old, f_old, part);
        });
    const unsigned col_blocks = (flags & UPDATE_Q) ? (unsigned)adm_fold_col_blocks(ncols, KT) : 0u;
    launch(ADM_FOLD_THREADS, col_blocks + 1, 1, [&] { k_adm_fold<KT>(part, splits, ncols, q_old, q_new, ll_a, ll_b, n_ll, out); });
}

// one iteration as snpm_panel_admix launches it
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, int64_t row0, int64_t n_rows, int K, unsigned flags,
                     Fill fill = RANDOM)
{
    Panel p = make_panel(lay, n_snp, n_acc, kStyle);
    if (fill != RANDOM) {                   // rewrite the calls: all missing; every fifth call of an int8 panel "other"; blank rows 1, 2 and column 0
        for (int64_t r = 0; r < n_snp; ++r)
            for (int64_t a = 0; a < n_acc; ++a) {
                int8_t &c = p.calls[(size_t)(r * n_acc + a)];
                if (fill == ALL_MISSING || (fill == BLANK_ROWS_AND_COLUMNS && (r == 1 || r == 2 || a == 0))) c = -1;
                if (fill == WITH_CODE3 && (r + a) % 5 == 0) c = 3;
            }
        for (int64_t r = 0; r < n_snp; ++r)              // re-encode the rewritten calls into the layout's bytes
            for (int64_t b = 0; b < (p.packed ? (n_acc + 3) / 4 : n_acc); ++b) {
                if (!p.packed) {
                    const int8_t c = p.calls[(size_t)(r * n_acc + b)];
                    p.d[r * p.pitch + b] = c >= 0 ? c : (int8_t)(0x80 | (rnd() & 0x7F));
                    continue;
                }
                unsigned out = 0;
                for (int f = 0; f < 4; ++f) {
                    const int64_t a = 4 * b + f;
                    const int v = a < n_acc ? p.calls[(size_t)(r * n_acc + a)] : (int)(rnd() & 3) - 1;
                    out |= (unsigned)(v < 0 ? 3 : v) << (2 * f);
                }
                ((uint8_t *)p.d)[pk_off(p.pitch, p.desc, r, b)] = (uint8_t)out;
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
    const int64_t first = rows ? 0 : row0;
    const int kt = adm_pitch(K);
    const size_t q_doubles = (size_t)(ncols * kt), f_doubles = (size_t)(n_rows * kt);
    double *q_old = (double *)exact_block(q_doubles * 8), *q_new = (double *)exact_block(q_doubles * 8);
    double *f_old = (double *)exact_block(f_doubles * 8), *f_new = (double *)exact_block(f_doubles * 8);
    memset(q_old, 0, q_doubles * 8); memset(q_new, 0, q_doubles * 8);          // (the library zeroes both copies: the entries beyond K)
    memset(f_old, 0, f_doubles * 8); memset(f_new, 0, f_doubles * 8);
    for (int64_t i = 0; i < ncols; ++i) {
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += q_old[i * kt + k] = (i % 7 == 3 && k == 0 && K > 1) ? 0.0 : -std::log(unit());      // (a zero entry now and then)
        for (int k = 0; k < K; ++k) q_old[i * kt + k] /= sum;
    }
    for (int64_t s = 0; s < n_rows; ++s)
        for (int k = 0; k < K; ++k) {
            const uint32_t pick = rnd() % 16;
            f_old[s * kt + k] = pick == 0 ? SNPM_ADMIX_EPS : pick == 1 ? 1.0 - SNPM_ADMIX_EPS : 0.02 + 0.96 * unit();
        }
    const int64_t n_ll = adm_ll_blocks(n_rows), splits = adm_splits(n_rows, ncols);
    const size_t part_bytes = (size_t)splits * q_doubles * 8, llb = (size_t)((n_ll + ADM_TREE_RADIX - 1) / ADM_TREE_RADIX);
    double *part = (double *)exact_block(part_bytes), *ll_a = (double *)exact_block((size_t)n_ll * 8), *ll_b = (double *)exact_block(llb * 8);
    double *out = (double *)exact_block(8);
    memset(part, 0x5A, part_bytes); memset(ll_a, 0x5A, (size_t)n_ll * 8); memset(ll_b, 0x5A, llb * 8); memset(out, 0x5A, 8);      // stale contents
    switch (kt) {
    case 4: launch_iteration<4>(p, rows, first, n_rows, cols, ncols, K, flags, q_old, q_new, f_old, f_new, part, ll_a, ll_b, out); break;
    case 8: launch_iteration<8>(p, rows, first, n_rows, cols, ncols, K, flags, q_old, q_new, f_old, f_new, part, ll_a, ll_b, out); break;
    default: launch_iteration<16>(p, rows, first, n_rows, cols, ncols, K, flags, q_old, q_new, f_old, f_new, part, ll_a, ll_b, out); break;
    }
    // the plain loop, in long double
    typedef long double ld;
    std::vector<ld> a((size_t)(n_rows * K), 0), b((size_t)(n_rows * K), 0), c((size_t)(ncols * K), 0);
    ld ll = 0;
    int64_t cells = 0;
    for (int64_t s = 0; s < n_rows; ++s)
        for (int64_t i = 0; i < ncols; ++i) {
            const int8_t code = p.calls[(size_t)((rows ? rows[s] : row0 + s) * n_acc + (cols ? cols[i] : i))];
            if (code < 0 || code > 2) continue;
            ++cells;
            const ld g = code == 0 ? 0 : code == 1 ? 2 : 1;
            ld pp = 0, pb = 0;
            for (int k = 0; k < K; ++k) {
                pp += (ld)q_old[i * kt + k] * (ld)f_old[s * kt + k];
                pb += (ld)q_old[i * kt + k] * ((ld)1 - (ld)f_old[s * kt + k]);
            }
            const ld u = g / pp, v = ((ld)2 - g) / pb;
            if (g > 0) ll += g * std::log(pp);
            if (g < 2) ll += ((ld)2 - g) * std::log(pb);
            for (int k = 0; k < K; ++k) {
                a[(size_t)(s * K + k)] += u * (ld)q_old[i * kt + k];
                b[(size_t)(s * K + k)] += v * (ld)q_old[i * kt + k];
                c[(size_t)(i * K + k)] += u * (ld)f_old[s * kt + k] + v * ((ld)1 - (ld)f_old[s * kt + k]);
            }
        }
    const ld u52 = std::ldexp((ld)1, -52);
    long bad = 0;
    ld worst_f = 0, worst_q = 0;
    for (int64_t s = 0; s < n_rows; ++s)
        for (int k = 0; k < kt; ++k) {
            const double got = f_new[s * kt + k];
            if (k >= K || !(flags & UPDATE_F)) { bad += got != 0.0; continue; }      // not written: the zeros of the start
            const ld f = f_old[s * kt + k], x = f * a[(size_t)(s * K + k)], den = x + ((ld)1 - f) * b[(size_t)(s * K + k)];
            if (den == 0) { bad += got != f_old[s * kt + k]; continue; }
            ld want = x / den;
            want = want < (ld)SNPM_ADMIX_EPS ? (ld)SNPM_ADMIX_EPS : want > (ld)(1.0 - SNPM_ADMIX_EPS) ? (ld)(1.0 - SNPM_ADMIX_EPS) : want;
            const ld ratio = std::fabs((ld)got - want) / want / ((ld)(ncols + 64) * u52);
            worst_f = std::max(worst_f, ratio);
            bad += !(ratio <= 1);
        }
    for (int64_t i = 0; i < ncols; ++i) {
        ld sum = 0;
        for (int k = 0; k < K; ++k) sum += (ld)q_old[i * kt + k] * c[(size_t)(i * K + k)];
        for (int k = 0; k < kt; ++k) {
            const double got = q_new[i * kt + k];
            if (!(flags & UPDATE_Q)) { bad += got != 0.0; continue; }
            if (k >= K) { bad += got != 0.0; continue; }
            if (sum == 0) { bad += got != q_old[i * kt + k]; continue; }
            const ld want = (ld)q_old[i * kt + k] * c[(size_t)(i * K + k)] / sum;
            if (want == 0) { bad += got != 0.0; continue; }
            const ld ratio = std::fabs((ld)got - want) / want / ((ld)(n_rows + 64) * u52);
            worst_q = std::max(worst_q, ratio);
            bad += !(ratio <= 1);
        }
    }
    const ld ll_bound = u52 * ((ld)(K + 2) * (ld)cells + (ld)((ncols + 63) / 64 + 64) * std::fabs(ll));
    const ld ratio_ll = ll_bound > 0 ? std::fabs((ld)out[0] - ll) / ll_bound : (out[0] == 0.0 ? 0 : 2);
    bad += !(ratio_ll <= 1);
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld K=%d flags=%u splits=%lld ll_blocks=%lld cells=%lld worst_f=%.3f worst_q=%.3f worst_ll=%.3f %s\n", name, (int)lay,
           (long long)n_acc, (long long)ncols, (long long)n_rows, K, flags, (long long)splits, (long long)n_ll, (long long)cells, (double)worst_f, (double)worst_q,
           (double)ratio_ll, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(out); free(ll_b); free(ll_a); free(part); free(f_new); free(f_old); free(q_new); free(q_old); free(rows); free(cols); free(p.d);
}

static void plan_case(const char *name, int64_t got, int64_t want)
{
    printf("case %s got=%lld want=%lld %s\n", name, (long long)got, (long long)want, got == want ? "ok" : "MISMATCH");
    g_fails += got != want;
}

int main()
{
    const int ks[8] = {1, 2, 3, 4, 5, 8, 9, 16};
    const unsigned fl[4] = {UPDATE_F | UPDATE_Q, UPDATE_F, UPDATE_Q, 0u};
    int n = 0;
    // every width with two of the row counts -- around a wave's run of 8 rows, a block of 32, a chunk and the shortest split of 16 --
    // in turn; the layouts, K and the flags rotate with them
    const int64_t row_counts[10] = {1, 15, 16, 17, 63, 64, 65, 1023, 1025, 2500};
    for (int64_t acc : {1, 2, 63, 64, 65, 129, 130, 255, 256, 257})
        for (int pick = 0; pick < 2; ++pick) {
            const int64_t rows = row_counts[n % 10];
            run_case("grid", (Layout)(n % 3), rows + 3, acc, 0, 0, 3, rows, ks[n % 8], fl[n % 7 == 6 ? 3 : n % 3 == 2 ? 1 + n % 2 : 0]);
            ++n;
        }
    // the split boundary of k_adm_cols: one column block wants 512 splits of at least 16 rows (8192 rows), two column blocks want 256 (4096)
    for (int64_t rows : {8191, 8192, 8193}) run_case("split-edge-1", (Layout)(rows % 3), rows, 3, 0, 0, 0, rows, 2, UPDATE_F | UPDATE_Q);
    for (int64_t rows : {4095, 4096, 4097}) run_case("split-edge-2", (Layout)(rows % 3), rows, 257, 0, 0, 0, rows, 3, UPDATE_Q);
    // column lists in descending order with a repeat, row lists unsorted with repeats; a dense range that does not start at row 0
    run_case("lists", INT8, 300, 70, 1, 1, 0, 200, 5, UPDATE_F | UPDATE_Q);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, 0, 129, 2, UPDATE_F | UPDATE_Q);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, 0, 129, 16, UPDATE_F | UPDATE_Q);
    run_case("row0", INT8, 200, 33, 0, 0, 57, 143, 9, UPDATE_F | UPDATE_Q);
    run_case("all-missing", PACKED, 70, 33, 0, 0, 0, 70, 3, UPDATE_F | UPDATE_Q, ALL_MISSING);
    run_case("blank-rows-columns", SPLIT, 70, 33, 0, 0, 0, 70, 4, UPDATE_F | UPDATE_Q, BLANK_ROWS_AND_COLUMNS);
    run_case("code3", INT8, 130, 65, 0, 0, 0, 130, 8, UPDATE_F | UPDATE_Q, WITH_CODE3);
    run_case("evaluate-only", PACKED, 130, 65, 0, 0, 0, 130, 8, 0u);
    // the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28), five column blocks
    run_case("split-wide", SPLIT, 40, 1135, 0, 0, 0, 40, 8, UPDATE_F | UPDATE_Q);
    // the plans alone
    plan_case("plan-pitch", adm_pitch(1) * 10000 + adm_pitch(4) * 1000 + adm_pitch(5) * 100 + adm_pitch(8) * 10 + adm_pitch(9) + adm_pitch(16), 4 * 10000 + 4 * 1000 + 8 * 100 + 8 * 10 + 16 + 16);
    plan_case("plan-split-rows-min", adm_split_rows(8192, 256), 16);
    plan_case("plan-split-rows-grow", adm_split_rows(8193, 256), 17);
    plan_case("plan-splits-1135", adm_splits(200000, 1135), (200000 + 1941) / 1942);
    plan_case("plan-splits-short", adm_splits(17, 1135), 2);
    plan_case("plan-ll-blocks", adm_ll_blocks(33), 2);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
