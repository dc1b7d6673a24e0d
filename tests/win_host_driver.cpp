// The kernel source of csrc/snpm_k_win.hpp compiled for the host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header,
// tests/host_kernel/harness.hpp runs it) with its launch geometry: every block by 256 real threads with a barrier for __syncthreads,
// the ballots and shuffles of a wave through its 64 threads.  Built with -fsanitize=address,undefined by tests/test_windows_cpu.py
// and run as a child process: the panel, the row and column lists, the pair lists, the offset table, the planes and the cells are
// heap blocks of exactly the size the library would use, the pad bytes of the rows hold arbitrary values and the workspaces start
// with stale contents; the slab plan is the library's own (win_slab_steps) and the cells of a slab are added into zeroed results as
// the library adds them.  Every count is compared with a brute-force count.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;

enum Table { EDGES, ONE, SPAN, RANDOM };

// EDGES: an empty window first, window edges at bits 0, 1, 63, 64 and 65 of a word, an empty window in the middle, a one-row
// window, the rest in one window and an empty window last.  ONE: all rows in one window.  SPAN: windows of 700 rows from row 300 on
// (every edge of a 1024-row plane step lies inside one) after a window of 1500 rows when the rows allow it.  RANDOM: random cuts.
static std::vector<int64_t> make_table(Table t, int64_t n_rows)
{
    std::vector<int64_t> off = {0};
    auto cut = [&](int64_t at) { off.push_back(std::max(off.back(), std::min(at, n_rows))); };
    if (t == EDGES) {
        for (int64_t at : {0, 1, 63, 64, 65, 65, 66, 127, 129, 192}) cut(at);
        cut(n_rows); cut(n_rows);
    } else if (t == ONE) {
        cut(n_rows);
    } else if (t == SPAN) {
        cut(300);
        if (n_rows > 4000) cut(1800);
        while (off.back() < n_rows) cut(off.back() + 700);
    } else {
        const int n = 1 + (int)(rnd() % 9);
        std::vector<int64_t> cuts;
        for (int k = 0; k < n; ++k) cuts.push_back((int64_t)(rnd() % (uint32_t)(n_rows + 1)));
        std::sort(cuts.begin(), cuts.end());
        for (int64_t c : cuts) cut(c);
        cut(n_rows);
    }
    return off;
}

// the launches of snpm_panel_window_counts, with `ws_bytes` as the workspace budget.  outs: 1 = columns, 2 = pairs, 3 = both
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int64_t n_rows, Table table, int use_cols, int use_rows, int outs,
                     size_t ws_bytes)
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
    if (use_rows) {                         // unsorted, with a repeat
        rows = (int64_t *)exact_block((size_t)std::max<int64_t>(1, n_rows) * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = (int64_t)(rnd() % n_snp);
        if (n_rows > 2) rows[n_rows - 1] = rows[0];
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    // pairs: (a, a), (a, b) and (b, a) among random ones
    const int64_t n_pairs = (outs & 2) ? 5 : 0;
    int32_t *pa = n_pairs ? (int32_t *)exact_block((size_t)n_pairs * 4) : nullptr, *pb = n_pairs ? (int32_t *)exact_block((size_t)n_pairs * 4) : nullptr;
    for (int64_t i = 0; i < n_pairs; ++i) { pa[i] = (int32_t)(rnd() % ncols); pb[i] = (int32_t)(rnd() % ncols); }
    if (n_pairs) { pb[0] = pa[0]; pa[2] = pb[1]; pb[2] = pa[1]; }
    const std::vector<int64_t> off_v = make_table(table, n_rows);
    const int64_t n_win = (int64_t)off_v.size() - 1;
    int64_t *win_off = (int64_t *)exact_block((size_t)(n_win + 1) * sizeof(int64_t));
    memcpy(win_off, off_v.data(), (size_t)(n_win + 1) * sizeof(int64_t));
    const int64_t acc_cols = (outs & 1) ? ncols : 0;
    int32_t *acc = (int32_t *)calloc((size_t)std::max<int64_t>(1, n_win * ncols * 4), sizeof(int32_t));
    int32_t *pair = (int32_t *)calloc((size_t)std::max<int64_t>(1, n_pairs * n_win * 4), sizeof(int32_t));
    int slabs = 0, lgs = 0;
    if (n_rows > 0) {
        const int64_t cols_pad = (ncols + WN_PL_COLS - 1) / WN_PL_COLS * WN_PL_COLS, cell_bytes = 16 * (acc_cols + n_pairs);
        for (int64_t s0 = 0, w_lo = 0, w_end = 0; s0 < n_rows; ++slabs) {
            const int64_t steps = win_slab_steps(ws_bytes, cols_pad, cell_bytes, win_off, n_win, n_rows, s0, w_lo, w_end), n_w = w_end - w_lo;
            const int64_t n_valid = std::min(steps * WN_STEP_ROWS, n_rows - s0);
            const int64_t W = (n_valid + WN_STEP_ROWS - 1) / WN_STEP_ROWS * WN_STEP_WORDS;
            const size_t plane_bytes = (size_t)(steps * win_step_bytes(cols_pad)), items = (size_t)(n_w * (acc_cols + n_pairs));
            unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
            int32_t *cells = (int32_t *)exact_block(items * 16);
            memset(planes, 0xA5, plane_bytes);                        // stale contents
            memset(cells, 0xA5, items * 16);
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab, as in the library
            int64_t *slab_list = nullptr;
            if (rows) {
                slab_list = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(slab_list, rows + s0, (size_t)n_valid * sizeof(int64_t));
            }
            launch(WN_THREADS, (unsigned)W, (unsigned)(cols_pad / WN_PL_COLS), [&] {
                k_win_planes(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, ncols, planes, cols_pad, W);
            });
            const int lg = win_group_lg(n_valid, n_w);
            lgs |= 1 << lg;
            const int64_t per_block = WN_THREADS >> lg, blocks = ((int64_t)items + per_block - 1) / per_block;
            launch(WN_THREADS, (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 3)), 1, [&] {      // three blocks: the stride loop runs
                k_win_count(planes, cols_pad, W, s0, n_valid, win_off, w_lo, n_w, acc_cols, pa, pb, n_pairs, lg, cells);
            });
            const int32_t *src = cells;
            if (acc_cols) {
                for (int64_t k = 0; k < n_w * ncols * 4; ++k) acc[w_lo * ncols * 4 + k] += src[k];
                src += n_w * ncols * 4;
            }
            for (int64_t i = 0; i < n_pairs; ++i)
                for (int64_t k = 0; k < n_w * 4; ++k) pair[(i * n_win + w_lo) * 4 + k] += src[i * n_w * 4 + k];
            free(slab_list); free(planes); free(cells);
            s0 += steps * WN_STEP_ROWS;
        }
    }
    // brute force
    long bad = 0;
    auto call = [&](int64_t r, int64_t c) { return (int)p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + (cols ? cols[c] : c))]; };
    for (int64_t w = 0; w < n_win; ++w) {
        for (int64_t c = 0; c < acc_cols; ++c) {
            int32_t want[4] = {0, 0, 0, 0};
            for (int64_t r = win_off[w]; r < win_off[w + 1]; ++r) {
                const int x = call(r, c);
                if (x >= 0 && x <= 2) ++want[x];
                want[3] += x >= 0;
            }
            for (int q = 0; q < 4; ++q) bad += acc[(w * ncols + c) * 4 + q] != want[q];
        }
        for (int64_t i = 0; i < n_pairs; ++i) {
            int32_t want[4] = {0, 0, 0, 0};
            for (int64_t r = win_off[w]; r < win_off[w + 1]; ++r) {
                const int x = call(r, pa[i]), y = call(r, pb[i]);
                if (x < 0 || x > 2 || y < 0 || y > 2) continue;
                ++want[0];
                want[1] += x == y;
                if (x <= 1 && y <= 1) ++want[x == y ? 2 : 3];
            }
            for (int q = 0; q < 4; ++q) bad += pair[(i * n_win + w) * 4 + q] != want[q];
        }
    }
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld windows=%lld table=%d list=%d outs=%d slabs=%d lgs=%d %s\n", name, (int)lay, (long long)n_acc,
           (long long)ncols, (long long)n_rows, (long long)n_win, (int)table, use_rows, outs, slabs, lgs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(acc); free(pair); free(win_off); free(pa); free(pb); free(rows); free(cols); free(p.d);
}

// the plan alone, on the table win_off[w] = min(w * stride, n_rows), win_off[n_win] = n_rows: "s0:steps:w_lo:n_w" per slab, for
// engine.window_slabs to agree with
static void plan_case(size_t ws_bytes, int64_t ncols, int64_t cells, int64_t n_rows, int64_t stride, int64_t n_win)
{
    std::vector<int64_t> off((size_t)n_win + 1);
    for (int64_t w = 0; w < n_win; ++w) off[(size_t)w] = std::min(w * stride, n_rows);
    off[(size_t)n_win] = n_rows;
    const int64_t cols_pad = (ncols + WN_PL_COLS - 1) / WN_PL_COLS * WN_PL_COLS;
    std::string plan;
    int64_t covered = 0;
    for (int64_t s0 = 0, w_lo = 0, w_end = 0; s0 < n_rows;) {
        const int64_t steps = win_slab_steps(ws_bytes, cols_pad, 16 * cells, off.data(), n_win, n_rows, s0, w_lo, w_end);
        plan += (plan.empty() ? "" : ",") + std::to_string(s0) + ":" + std::to_string(steps) + ":" + std::to_string(w_lo) + ":" + std::to_string(w_end - w_lo);
        covered += std::min(steps * WN_STEP_ROWS, n_rows - s0);
        s0 += steps * WN_STEP_ROWS;
    }
    printf("case plan ws=%llu ncols=%lld cells=%lld rows=%lld stride=%lld nwin=%lld slabs=%s %s\n", (unsigned long long)ws_bytes, (long long)ncols, (long long)cells,
           (long long)n_rows, (long long)stride, (long long)n_win, plan.c_str(), covered == n_rows ? "ok" : "MISMATCH");
    g_fails += covered != n_rows;
}

int main()
{
    const size_t big = size_t(256) << 20;
    int k = 0;
    // every width over the four layouts, the edge table: all edges of a word, the empty windows, the one-row window
    for (int64_t acc : {1, 2, 63, 64, 65, 130, 1135})
        for (int lay = 0; lay < 4; ++lay) {
            run_case("edges", (Layout)lay, 203, acc, 200, EDGES, 0, 0, 1 + k % 3, big);
            ++k;
        }
    // short selections: no row, one row, one word and one row more
    for (int64_t rows : {0, 1, 64, 65}) run_case("short", (Layout)(k++ % 3), rows + 3, 33, rows, EDGES, 0, 0, 3, big);
    // one window holding all rows; columns only and pairs only; a window longer than a plane step
    run_case("one-window", PACKED, 2200, 65, 2200, ONE, 0, 0, 3, big);       // 35 words: a whole wave per cell
    run_case("one-short-window", INT8, 200, 5, 200, ONE, 0, 0, 3, big);      // 4 words: four lanes per cell
    run_case("columns-only", INT8, 1300, 7, 1300, ONE, 0, 0, 1, big);         // 21 words: 32 lanes per cell
    run_case("pairs-only", SPLIT, 90, 130, 90, RANDOM, 0, 0, 2, big);
    // a column list with a repeat, a row list that is unsorted with a repeat
    run_case("lists", INT8, 300, 70, 260, EDGES, 1, 1, 3, big);
    run_case("lists-split", SPLIT, 90, 1135, 129, RANDOM, 1, 1, 3, big);
    run_case("lists-tight", TIGHT, 120, 33, 200, RANDOM, 1, 1, 3, big);
    for (int r = 0; r < 4; ++r) run_case("random", (Layout)(r % 3), 700, 2 + 40 * r, 640, RANDOM, r & 1, r >> 1, 3, big);
    // two and three slabs (the budget holds one step): a window lies across every slab edge; one window over all slabs
    run_case("two-slabs", PACKED, 1500, 65, 1500, SPAN, 0, 0, 3, 1);
    run_case("three-slabs", INT8, 2110, 33, 2100, SPAN, 0, 0, 3, 1);
    run_case("list-three-slabs", SPLIT, 500, 130, 2100, SPAN, 1, 1, 3, 1);
    run_case("one-window-three-slabs", INT8, 2100, 2, 2100, ONE, 0, 0, 3, 1);
    run_case("edges-two-slabs", PACKED, 1100, 7, 1100, EDGES, 0, 0, 3, 1);
    // a budget that holds two steps of 64 padded columns and some cells: slabs of two steps, a long window first
    run_case("two-step-slabs", INT8, 4500, 40, 4500, SPAN, 0, 0, 3, (size_t)(2 * win_step_bytes(64) + 16 * 45 * 4));
    // the arithmetic of the plan
    plan_case(size_t(1) << 20, 1135, 1235, 11000, 28, 399);
    plan_case(size_t(256) << 20, 1135, 1235, 11000000, 27569, 399);
    plan_case(1, 1, 1, 10, 3, 5);
    plan_case(size_t(1) << 20, 64, 64, 5000, 1, 6000);
    plan_case(size_t(3) << 20, 200, 300, 70000, 5000, 20);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
