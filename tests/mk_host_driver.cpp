// The kernel source of csrc/snpm_k_mk.hpp compiled for the host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header,
// tests/host_kernel/harness.hpp runs it) with its launch geometry: every block by 256 real threads with a
// barrier for __syncthreads and an exchange per wave for __ballot / __shfl_xor.  Built with -fsanitize=address,undefined by
// tests/test_markers_cpu.py and run as a child process: the panel, the row and column lists, the planes, Ut, need, the gains, the block keys, the
// eligibility bytes, the coordinates, chosen / gain_at and the state are heap blocks of exactly the size the library would use, the
// pad bytes of the rows hold arbitrary values, every workspace starts with stale contents.  The launches are the library's: the
// planes, the initial need, then rounds of gain / pick / update in batches of MK_ROUND_BATCH with a look at the state between two
// batches -- so the rounds behind the end of the loop run too, and must change nothing.  The planes are compared with the calls,
// every result with a scalar greedy loop over rows and pairs, Ut with the final need.  Prints "case ... ok" per case and
// "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_mk.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;

enum Elig { ELIG_NULL, ELIG_RANDOM, ELIG_NOT_BEST, ELIG_NONE };
enum Rows { ROWS_RANGE, ROWS_LIST, ROWS_DUPLICATED };      // ROWS_DUPLICATED: a list in which every row comes twice in a row
enum Calls { CALLS_RANDOM, CALLS_MISSING, CALLS_HET, CALLS_ONE_ALLELE };

struct Case {
    const char *name;
    Layout lay;
    int64_t n_acc, n_rows;
    int depth;
    int64_t max_markers;        // < 0: the row count
    int use_cols;
    Rows rows;
    Elig elig;
    int coord;                  // 0: none; 1: random in 0 .. 49; 2: every coordinate twice
    int64_t min_dist;
    Calls calls;
};

static void run_case(const Case &c)
{
    const int64_t n_snp = c.n_rows + 5, n_rows = c.n_rows;
    Panel p = make_panel(c.lay, n_snp, c.n_acc, kStyle);
    if (c.calls != CALLS_RANDOM) {          // a degenerate panel: written into the calls and the device bytes alike
        const int8_t v = c.calls == CALLS_MISSING ? -1 : c.calls == CALLS_HET ? 2 : 1;
        for (int64_t r = 0; r < n_snp; ++r)
            for (int64_t a = 0; a < c.n_acc; ++a) {
                p.calls[(size_t)(r * c.n_acc + a)] = v;
                if (!p.packed) {
                    p.d[r * p.pitch + a] = v;
                } else {
                    uint8_t *byte = (uint8_t *)p.d + pk_off(p.pitch, p.desc, r, a >> 2);
                    *byte = (uint8_t)((*byte & ~(3u << (2 * (a & 3)))) | ((unsigned)(v < 0 ? 3 : v) << (2 * (a & 3))));
                }
            }
    }
    int64_t ncols = c.n_acc, row0 = 0;
    int32_t *cols = nullptr;
    int64_t *rows = nullptr;
    if (c.use_cols) {                       // a shuffled subset with one repeat
        ncols = std::max<int64_t>(2, c.n_acc - c.n_acc / 3);
        cols = (int32_t *)exact_block((size_t)ncols * sizeof(int32_t));
        for (int64_t a = 0; a < ncols; ++a) cols[a] = (int32_t)(rnd() % c.n_acc);
        cols[ncols - 1] = cols[0];
    }
    if (c.rows != ROWS_RANGE) {
        rows = (int64_t *)exact_block((size_t)n_rows * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = c.rows == ROWS_DUPLICATED && (r & 1) ? rows[r - 1] : (int64_t)(rnd() % n_snp);
        if (c.rows == ROWS_LIST && n_rows > 1) rows[n_rows - 1] = rows[0];
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    const int64_t cols_pad = (ncols + WAVE - 1) / WAVE * WAVE;
    const int Wc = (int)(cols_pad / WAVE);
    const int64_t max_markers = c.max_markers < 0 ? n_rows : c.max_markers, cap = std::min(max_markers, n_rows);
    auto code = [&](int64_t r, int64_t a) { return (int)p.calls[(size_t)((rows ? rows[r] : row0 + r) * c.n_acc + (cols ? cols[a] : a))]; };
    // ---- the device's buffers, stale
    const size_t h_words = (size_t)(n_rows * 2 * Wc), ut_words = (size_t)(Wc * cols_pad), cells = (size_t)(ncols * ncols);
    unsigned long long *H = (unsigned long long *)exact_block(h_words * 8), *Ut = (unsigned long long *)exact_block(ut_words * 8);
    uint8_t *need = (uint8_t *)exact_block(cells), *elig = (uint8_t *)exact_block((size_t)n_rows);
    int32_t *gain = (int32_t *)exact_block((size_t)n_rows * 4), *first_gain = (int32_t *)exact_block((size_t)n_rows * 4);
    int64_t *chosen = (int64_t *)exact_block((size_t)cap * 8), *coord = nullptr;
    int32_t *gain_at = (int32_t *)exact_block((size_t)cap * 4);
    MkState *st = (MkState *)exact_block(sizeof(MkState));
    const int64_t n_best = (n_rows + MK_GAIN_ROWS - 1) / MK_GAIN_ROWS;
    unsigned long long *best = (unsigned long long *)exact_block((size_t)n_best * 8);
    memset(best, 0xA5, (size_t)n_best * 8);
    memset(H, 0xA5, h_words * 8); memset(Ut, 0x5A, ut_words * 8); memset(need, 0xA5, cells); memset(gain, 0x7F, (size_t)n_rows * 4);
    memset(chosen, 0xA5, (size_t)cap * 8); memset(gain_at, 0xA5, (size_t)cap * 4);
    if (c.coord) {
        coord = (int64_t *)exact_block((size_t)n_rows * 8);
        for (int64_t r = 0; r < n_rows; ++r) coord[r] = c.coord == 2 ? 1000 - r / 2 : (int64_t)(rnd() % 50) - 25;
    }
    // ---- the planes, then the scalar answer (the eligibility mask of ELIG_NOT_BEST needs round 0's gains)
    launch(MK_THREADS, (unsigned)((n_rows + MK_PL_ROWS - 1) / MK_PL_ROWS), 1, [&] {
        k_mk_rowplanes(p.d, p.pitch, p.desc, rows, row0, n_rows, cols, (int)ncols, H, Wc);
    });
    long bad = 0;
    for (int64_t r = 0; r < n_rows; ++r)
        for (int pl = 0; pl < 2; ++pl)
            for (int w = 0; w < Wc; ++w) {
                unsigned long long want = 0;
                for (int64_t a = (int64_t)w * 64; a < std::min<int64_t>(ncols, (int64_t)w * 64 + 64); ++a) want |= (unsigned long long)(code(r, a) == pl) << (a & 63);
                bad += H[(size_t)((r * 2 + pl) * Wc + w)] != want;
            }
    auto separates = [&](int64_t r, int64_t a, int64_t b) { const int x = code(r, a), y = code(r, b); return (x == 0 && y == 1) || (x == 1 && y == 0); };
    std::vector<int> w_need(cells, 0);
    for (int64_t a = 0; a < ncols; ++a)
        for (int64_t b = 0; b < ncols; ++b) w_need[(size_t)(a * ncols + b)] = a == b ? 0 : c.depth;
    std::vector<int32_t> w_first((size_t)n_rows, 0);
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t a = 0; a < ncols; ++a)
            for (int64_t b = a + 1; b < ncols; ++b) w_first[(size_t)r] += separates(r, a, b);
    for (int64_t r = 0; r < n_rows; ++r) elig[r] = c.elig == ELIG_RANDOM ? (uint8_t)(rnd() % 4 ? 1 + rnd() % 255 : 0) : c.elig == ELIG_NONE ? 0 : 1;
    if (c.elig == ELIG_NOT_BEST && n_rows > 0) elig[std::max_element(w_first.begin(), w_first.end()) - w_first.begin()] = 0;
    std::vector<uint8_t> w_elig(elig, elig + n_rows);
    std::vector<int64_t> w_chosen;
    std::vector<int32_t> w_gain_at;
    long long w_remaining = (long long)c.depth * (ncols * (ncols - 1) / 2);
    int w_reason;
    for (;;) {
        if (w_remaining == 0) { w_reason = MK_STOP_RESOLVED; break; }
        if ((int64_t)w_chosen.size() == max_markers) { w_reason = MK_STOP_MAX_MARKERS; break; }
        int64_t top = -1;
        int32_t top_gain = 0;
        for (int64_t r = 0; r < n_rows; ++r) {
            if (!w_elig[(size_t)r]) continue;
            int32_t g = 0;
            for (int64_t a = 0; a < ncols; ++a)
                for (int64_t b = a + 1; b < ncols; ++b) g += w_need[(size_t)(a * ncols + b)] > 0 && separates(r, a, b);
            if (g > top_gain) { top = r; top_gain = g; }
        }
        if (top < 0) { w_reason = MK_STOP_NO_GAIN; break; }
        w_chosen.push_back(top);
        w_gain_at.push_back(top_gain);
        for (int64_t a = 0; a < ncols; ++a)
            for (int64_t b = 0; b < ncols; ++b)
                if (a != b && w_need[(size_t)(a * ncols + b)] > 0 && separates(top, a, b)) --w_need[(size_t)(a * ncols + b)];
        w_remaining -= top_gain;
        w_elig[(size_t)top] = 0;
        for (int64_t r = 0; r < n_rows && coord; ++r) {
            const int64_t d = coord[r] - coord[top];
            if ((d < 0 ? -d : d) < c.min_dist) w_elig[(size_t)r] = 0;
        }
    }
    // ---- the library's launches
    *st = MkState{0, (long long)c.depth * (ncols * (ncols - 1) / 2), -1, 0, 0};
    const unsigned upd_grid = (unsigned)(cols_pad / (MK_THREADS / WAVE));
    launch(MK_THREADS, upd_grid, 1, [&] { k_mk_update(H, n_rows, Wc, (int)ncols, cols_pad, st, -1, c.depth, need, Ut); });
    int64_t rounds = 0;
    int batches = 0;
    while (rounds < cap) {
        const int64_t upto = std::min<int64_t>(cap, rounds + MK_ROUND_BATCH);
        for (; rounds < upto; ++rounds) {
            const int64_t round = rounds;
            launch(MK_THREADS, (unsigned)n_best, 1, [&] {
                k_mk_gain(H, Ut, elig, st, n_rows, cols_pad, Wc, round == 0, gain, best);
            });
            if (round == 0) memcpy(first_gain, gain, (size_t)n_rows * 4);
            launch(MK_PICK_THREADS, 1, 1, [&] { k_mk_pick(best, n_best, elig, coord, c.min_dist, n_rows, max_markers, cap, chosen, gain_at, st); });
            launch(MK_THREADS, upd_grid, 1, [&] { k_mk_update(H, n_rows, Wc, (int)ncols, cols_pad, st, round, 0, need, Ut); });
        }
        ++batches;
        if (st->done) break;
    }
    int reason = st->reason;
    if (!st->done) reason = MK_STOP_NO_GAIN;        // (the library: every row was picked and pairs are left)
    // ---- compare
    bad += st->n_chosen != (long long)w_chosen.size() || st->remaining != w_remaining || reason != w_reason;
    if (!st->done) bad += !(st->n_chosen == n_rows && n_rows < max_markers && st->remaining > 0);
    for (size_t k = 0; k < w_chosen.size() && (long long)k < st->n_chosen; ++k) bad += chosen[k] != w_chosen[k] || gain_at[k] != w_gain_at[k];
    for (size_t k = 0; k < cells; ++k) bad += need[k] != w_need[k];
    for (int64_t r = 0; r < n_rows && cap > 0; ++r) bad += first_gain[r] != w_first[(size_t)r];
    for (int w = 0; w < Wc; ++w)
        for (int64_t a = 0; a < cols_pad; ++a) {
            unsigned long long want = 0;
            for (int64_t b = (int64_t)w * 64; a < ncols && b < std::min<int64_t>(ncols, (int64_t)w * 64 + 64); ++b)
                want |= (unsigned long long)(w_need[(size_t)(a * ncols + b)] > 0) << (b & 63);
            bad += Ut[(size_t)(w * cols_pad + a)] != want;
        }
    for (int64_t r = 0; r < n_rows; ++r) bad += (elig[r] != 0) != (w_elig[(size_t)r] != 0);
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld depth=%d max=%lld picks=%lld remaining=%lld reason=%d rounds=%lld batches=%d %s\n", c.name, (int)c.lay,
           (long long)c.n_acc, (long long)ncols, (long long)n_rows, c.depth, (long long)max_markers, (long long)w_chosen.size(), w_remaining, w_reason,
           (long long)rounds, batches, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(best); free(st); free(gain_at); free(chosen); free(coord); free(first_gain); free(gain); free(elig); free(need); free(Ut); free(H); free(rows); free(cols); free(p.d);
}

int main()
{
    int k = 0;
    // the edges of the accession bit words and of the ballot x the edges of a wave of rows and of a gain block's row group
    const int depths[4] = {1, 2, 3, 255};
    for (int64_t acc : {1, 2, 63, 64, 65, 130})
        for (int64_t rows : {1, MK_GAIN_ROWS - 1, MK_GAIN_ROWS, MK_GAIN_ROWS + 1, 63, 64, 65}) {
            const int depth = depths[k % 4];
            // (two rounds in two cases of three: a round costs three launches of 256 real threads each here)
            run_case({"grid", (Layout)(k % 3), acc, rows, depth, k % 3 ? 2 : rows > MK_GAIN_ROWS + 1 ? MK_ROUND_BATCH + 2 : -1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
            ++k;
        }
    // selections: a shuffled row list with repeats, a column list with a repeat (a pair nothing separates), in every layout
    for (int lay = 0; lay < 3; ++lay) run_case({"lists", (Layout)lay, 70, 24, 1, -1, 1, ROWS_LIST, ELIG_NULL, 0, 0, CALLS_RANDOM});
    // eligibility masks: a random one, one that forbids the row with the largest gain
    run_case({"masked", PACKED, 20, 16, 2, -1, 0, ROWS_RANGE, ELIG_RANDOM, 0, 0, CALLS_RANDOM});
    run_case({"not-best", SPLIT, 33, 12, 1, -1, 0, ROWS_RANGE, ELIG_NOT_BEST, 0, 0, CALLS_RANDOM});
    // max_markers: 1, the end of a batch of rounds, one more
    run_case({"max-1", INT8, 40, 30, 1, 1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
    run_case({"max-batch", PACKED, 130, 40, 3, MK_ROUND_BATCH, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
    run_case({"max-batch-plus-1", SPLIT, 130, 40, 3, MK_ROUND_BATCH + 1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
    // coordinates: a min_dist larger than the whole range (one pick), min_dist 1 with every coordinate twice, a middle value
    run_case({"dist-all", INT8, 20, 40, 1, -1, 0, ROWS_RANGE, ELIG_NULL, 1, 1000, CALLS_RANDOM});
    run_case({"dist-1-twice", PACKED, 20, 20, 2, -1, 0, ROWS_RANGE, ELIG_NULL, 2, 1, CALLS_RANDOM});
    run_case({"dist-5", SPLIT, 33, 30, 1, -1, 0, ROWS_LIST, ELIG_RANDOM, 1, 5, CALLS_RANDOM});
    run_case({"dist-0", INT8, 12, 20, 1, -1, 0, ROWS_RANGE, ELIG_NULL, 1, 0, CALLS_RANDOM});
    // duplicate rows: the second copy has no gain after the first pick at depth 1 and is picked at depth 2
    run_case({"duplicated-depth-1", INT8, 12, 16, 1, -1, 0, ROWS_DUPLICATED, ELIG_NULL, 0, 0, CALLS_RANDOM});
    run_case({"duplicated-depth-2", PACKED, 12, 12, 2, -1, 0, ROWS_DUPLICATED, ELIG_NULL, 0, 0, CALLS_RANDOM});
    // depth 255: need never reaches 0, every row with gain is picked once, the loop ends with every row picked
    run_case({"depth-255", INT8, 9, 10, 255, -1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
    run_case({"depth-255-more-allowed", SPLIT, 9, 7, 255, 50, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
    // degenerate panels and masks
    run_case({"all-missing", PACKED, 65, 9, 1, -1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_MISSING});
    run_case({"all-het", INT8, 10, 9, 1, -1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_HET});
    run_case({"one-allele", SPLIT, 10, 9, 2, -1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_ONE_ALLELE});
    run_case({"nothing-eligible", INT8, 10, 9, 1, -1, 0, ROWS_RANGE, ELIG_NONE, 0, 0, CALLS_RANDOM});
    // the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28): 18 words per plane row
    run_case({"split-wide", SPLIT, 1135, 9, 1, 3, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
    // an end by the last pick that the host learns of at its second read of the state
    run_case({"resolved-in-batch-2", INT8, 10, 60, 4, -1, 0, ROWS_RANGE, ELIG_NULL, 0, 0, CALLS_RANDOM});
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
