// The kernel source of csrc/snpm_k_ibd.hpp (and k_win_planes of csrc/snpm_k_win.hpp, which it is launched behind) compiled for the
// host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header, tests/host_kernel/harness.hpp runs it) with its launch
// geometry: every block by 256 real threads with a barrier for __syncthreads.  Built with -fsanitize=address,undefined by
// tests/test_ibd_cpu.py and run as a child process: the panel, the row and column lists, the plan's tables, the planes, the
// matrices and the bitsets are heap blocks of exactly the size the library would use, the pad bytes of the rows hold arbitrary
// values, the planes, the three run matrices and the bitsets start with stale contents (the bitsets and the four totals are then
// zeroed as the library zeroes them); the plan (slabs, groups, segments) is the library's own (ibd_plan) and is checked on its own
// first: replayed bit by bit against the windows.  Every count, bit and run figure is compared with a brute-force count.  Prints
// "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

// what the host stand-in of the HIP header lacks for this family: a 32-bit atomic OR
inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"
#include "snpm_k_f1x.hpp"
#include "snpm_k_ibd.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;
typedef std::vector<int64_t> Offsets;

// ------------------------------------------------------------------------------------------------ window sets over n rows
static Offsets one_window(int64_t n) { return {0, n}; }
static Offsets every_row(int64_t n)
{
    Offsets o;
    for (int64_t k = 0; k <= n; ++k) o.push_back(k);
    return o;
}
static Offsets cuts(int64_t n, std::initializer_list<int64_t> at)      // boundaries at the listed rows, as far as they lie inside
{
    Offsets o{0};
    for (int64_t c : at) o.push_back(std::min(c, n));
    o.push_back(n);
    return o;
}
static Offsets every(int64_t n, int64_t len)
{
    Offsets o;
    for (int64_t k = 0; k < n; k += len) o.push_back(k);
    o.push_back(n);
    return o;
}

// the plan replayed: the segments of a slab's groups come window by window and word by word; every bit of a segment's mask is a row
// of the window its meta names, every row of a window with rows comes exactly once, the window's last segment -- and no other --
// carries the flag, no segment is empty; groups hold whole steps inside the slab's planes; an empty window has no segment
static long replay_plan(const IbdPlan &plan, const Offsets &off)
{
    long bad = 0;
    const int64_t n_win = (int64_t)off.size() - 1;
    std::vector<int64_t> seen((size_t)n_win, 0), ended((size_t)n_win, 0);
    int64_t prev_hi = 0, prev_win = -1;
    for (const IbdSlab &s : plan.slabs) {
        for (int64_t k = prev_hi; k < s.w_lo; ++k) bad += off[(size_t)k + 1] != off[(size_t)k];       // only empty windows between slabs
        prev_hi = s.w_hi;
        bad += s.r0 != off[(size_t)s.w_lo] || s.n_rows != off[(size_t)s.w_hi] - s.r0 || s.n_rows <= 0 || s.W != ibd_words(s.n_rows) || s.W > plan.max_W ||
               s.n_rows > plan.max_rows;
        for (int64_t g = s.g_lo; g < s.g_hi; ++g) {
            const int64_t gw0 = plan.groups[(size_t)(3 * g)], steps = plan.groups[(size_t)(3 * g + 1)], sb = plan.groups[(size_t)(3 * g + 2)];
            bad += gw0 % F1X_STEP_WORDS != 0 || steps < 1 || gw0 + steps * F1X_STEP_WORDS > s.W || sb + steps >= (int64_t)plan.step_off.size();
            for (int64_t st = 0; st < steps; ++st) {
                bad += plan.step_off[(size_t)(sb + st)] >= plan.step_off[(size_t)(sb + st + 1)];      // a group's steps all hold rows of its windows
                for (int64_t q = plan.step_off[(size_t)(sb + st)]; q < plan.step_off[(size_t)(sb + st + 1)]; ++q) {
                    const unsigned long long m = plan.segs[(size_t)(2 * q)], meta = plan.segs[(size_t)(2 * q + 1)];
                    const int64_t w = (int64_t)(meta >> IBD_SEG_WIN_SHIFT);
                    if (w < s.w_lo || w >= s.w_hi) { ++bad; continue; }
                    bad += m == 0 || (meta & 0xE0ull) != 0 || w < prev_win || ended[(size_t)w] != 0;
                    prev_win = w;
                    const int64_t word = gw0 + st * F1X_STEP_WORDS + (int64_t)(meta & 15);
                    for (int b = 0; b < 64; ++b)
                        if (m >> b & 1) {
                            const int64_t r = s.r0 + word * 64 + b;
                            bad += r < off[(size_t)w] || r >= off[(size_t)w + 1];
                            ++seen[(size_t)w];
                        }
                    if (meta & IBD_SEG_END) {
                        bad += seen[(size_t)w] != off[(size_t)w + 1] - off[(size_t)w];
                        ended[(size_t)w] = 1;
                    }
                }
            }
        }
    }
    for (int64_t w = 0; w < n_win; ++w) {
        const int64_t rows = off[(size_t)w + 1] - off[(size_t)w];
        bad += seen[(size_t)w] != rows || ended[(size_t)w] != (rows > 0);
    }
    return bad;
}

// the launches of snpm_panel_ibd_counts, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, const Offsets &off, int min_sites, int ppm,
                     int min_run, size_t ws_bytes, int want_slabs = 0, int want_groups = 0)
{
    const int64_t n_rows = off.back(), n_win = (int64_t)off.size() - 1, wwords = (n_win + 31) / 32;
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
    int64_t *win_off = (int64_t *)exact_block(off.size() * sizeof(int64_t));
    memcpy(win_off, off.data(), off.size() * sizeof(int64_t));
    const size_t cells = (size_t)(ncols * ncols), bit_words = cells * (size_t)wwords;
    int32_t *out = (int32_t *)exact_block(7 * cells * sizeof(int32_t));
    uint32_t *bits = (uint32_t *)exact_block(2 * bit_words * sizeof(uint32_t));
    memset(out, 0xA5, 7 * cells * sizeof(int32_t));                   // stale contents
    memset(bits, 0x5A, 2 * bit_words * sizeof(uint32_t));
    memset(out, 0, 4 * cells * sizeof(int32_t));                      // the library's two memsets: the four totals and the bitsets
    memset(bits, 0, 2 * bit_words * sizeof(uint32_t));
    long plan_bad = 0;
    int slabs = 0;
    int64_t n_groups = 0, n_segs = 0;
    {
        const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
        const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
        IbdPlan plan;
        ibd_plan(ws_bytes, cols_pad, win_off, n_win, plan);
        plan_bad = replay_plan(plan, off);
        slabs = (int)plan.slabs.size();
        n_groups = (int64_t)plan.groups.size() / IBD_GROUP_WORDS;
        n_segs = (int64_t)plan.segs.size() / IBD_SEG_WORDS;
        // the device's copies: exactly the bytes uploaded
        const size_t plane_bytes = (size_t)(F1X_PLANES * cols_pad * plan.max_W * 8);
        unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
        memset(planes, 0xA5, plane_bytes);                            // stale contents
        int64_t *d_groups = (int64_t *)exact_block(plan.groups.size() * sizeof(int64_t));
        int64_t *d_steps = (int64_t *)exact_block(plan.step_off.size() * sizeof(int64_t));
        unsigned long long *d_segs = (unsigned long long *)exact_block(plan.segs.size() * sizeof(unsigned long long));
        memcpy(d_groups, plan.groups.data(), plan.groups.size() * sizeof(int64_t));
        memcpy(d_steps, plan.step_off.data(), plan.step_off.size() * sizeof(int64_t));
        memcpy(d_segs, plan.segs.data(), plan.segs.size() * sizeof(unsigned long long));
        for (const IbdSlab &s : plan.slabs) {
            const int64_t first = rows ? 0 : row0 + s.r0;            // a row list travels slab by slab, as in the library
            const int64_t *slab_list = nullptr;
            if (rows) {
                int64_t *copy = (int64_t *)exact_block((size_t)s.n_rows * sizeof(int64_t));
                memcpy(copy, rows + s.r0, (size_t)s.n_rows * sizeof(int64_t));
                slab_list = copy;
            }
            launch(WN_THREADS, (unsigned)s.W, (unsigned)(cols_pad / F1X_PL_COLS), [&] {
                k_win_planes(p.d, p.pitch, p.desc, slab_list, first, s.n_rows, cols, ncols, planes, cols_pad, s.W);
            });
            if (s.g_hi > s.g_lo)
                launch(IBD_THREADS, (unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)(s.g_hi - s.g_lo), [&] {
                    k_ibd_count(planes, cols_pad, s.W, d_groups + s.g_lo * IBD_GROUP_WORDS, d_steps, d_segs, (int)ncols, n_tiles, min_sites, ppm, wwords, out,
                                out + cells, out + 2 * cells, out + 3 * cells, bits, bits + bit_words);
                });
            free((void *)slab_list);
        }
        if (n_rows > 0)                      // (no row: the library writes zeros itself, nothing is launched)
            launch(IBD_RUN_THREADS, (unsigned)((cells + IBD_RUN_THREADS - 1) / IBD_RUN_THREADS), 1, [&] {
                k_ibd_runs(bits, bits + bit_words, (int64_t)cells, wwords, min_run, out + 4 * cells, out + 5 * cells, out + 6 * cells);
            });
        free(d_segs); free(d_steps); free(d_groups); free(planes);
    }
    // brute force, every ordered cell on its own
    long bad = 0, shared_cells = 0, break_cells = 0;
    std::vector<int8_t> col_a((size_t)n_rows), col_b((size_t)n_rows);
    std::vector<uint32_t> ub((size_t)wwords), sb((size_t)wwords);
    for (int64_t a = 0; a < ncols && n_rows > 0; ++a) {
        const int64_t ca = cols ? cols[a] : a;
        for (int64_t r = 0; r < n_rows; ++r) col_a[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + ca)];
        for (int64_t b = 0; b < ncols; ++b) {
            const int64_t cb = cols ? cols[b] : b;
            for (int64_t r = 0; r < n_rows; ++r) col_b[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + cb)];
            int32_t w_used = 0, w_shared = 0, n_shared = 0, d_shared = 0, run_max = 0, n_runs = 0, w_in = 0, len = 0;
            std::fill(ub.begin(), ub.end(), 0u);
            std::fill(sb.begin(), sb.end(), 0u);
            auto close = [&] { run_max = std::max(run_max, len); if (len >= min_run) { ++n_runs; w_in += len; } len = 0; };
            for (int64_t w = 0; w < n_win; ++w) {
                int64_t n = 0, d = 0;
                for (int64_t r = off[(size_t)w]; r < off[(size_t)w + 1]; ++r) {
                    const int x = col_a[(size_t)r], y = col_b[(size_t)r];
                    if ((x != 0 && x != 1) || (y != 0 && y != 1)) continue;
                    ++n;
                    d += x != y;
                }
                if (n < min_sites) continue;
                ++w_used;
                ub[(size_t)(w >> 5)] |= 1u << (w & 31);
                if (d * 1000000 <= (int64_t)ppm * n) {
                    ++w_shared, ++len;
                    n_shared += (int32_t)n, d_shared += (int32_t)d;
                    sb[(size_t)(w >> 5)] |= 1u << (w & 31);
                } else {
                    close();
                }
            }
            close();
            const size_t at = (size_t)(a * ncols + b);
            bad += out[at] != w_used || out[cells + at] != w_shared || out[2 * cells + at] != n_shared || out[3 * cells + at] != d_shared ||
                   out[4 * cells + at] != run_max || out[5 * cells + at] != n_runs || out[6 * cells + at] != w_in;
            for (int64_t k = 0; k < wwords; ++k)
                bad += bits[at * (size_t)wwords + (size_t)k] != ub[(size_t)k] || bits[bit_words + at * (size_t)wwords + (size_t)k] != sb[(size_t)k];
            shared_cells += a != b && w_shared > 0;
            break_cells += w_used > w_shared;
        }
    }
    const bool plan_ok = (want_slabs == 0 || slabs == want_slabs) && (want_groups == 0 || n_groups == want_groups);
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld windows=%lld min=%d ppm=%d run=%d shared=%ld breaks=%ld slabs=%d groups=%lld segs=%lld %s\n", name,
           (int)lay, (long long)n_acc, (long long)ncols, (long long)n_rows, (long long)n_win, min_sites, ppm, min_run, shared_cells, break_cells, slabs,
           (long long)n_groups, (long long)n_segs, bad || plan_bad || !plan_ok ? "MISMATCH" : "ok");
    g_fails += bad != 0 || plan_bad != 0 || !plan_ok;
    free(bits); free(out); free(win_off); free(rows); free(cols); free(p.d);
}

// the plan alone: slabs, groups, steps and segments of a window set
static void plan_case(const char *name, const Offsets &off, size_t ws_bytes, int64_t cols_pad, int64_t want_slabs, int64_t want_groups, int64_t want_steps,
                      int64_t want_segs, int64_t want_max_rows)
{
    IbdPlan plan;
    ibd_plan(ws_bytes, cols_pad, off.data(), (int64_t)off.size() - 1, plan);
    const int64_t slabs = (int64_t)plan.slabs.size(), groups = (int64_t)plan.groups.size() / IBD_GROUP_WORDS;
    const int64_t steps = (int64_t)plan.step_off.size() - 1, segs = (int64_t)plan.segs.size() / IBD_SEG_WORDS;
    const bool ok = replay_plan(plan, off) == 0 && slabs == want_slabs && groups == want_groups && steps == want_steps && segs == want_segs &&
                    plan.max_rows == want_max_rows;
    printf("case plan-%s slabs=%lld groups=%lld steps=%lld segs=%lld max_rows=%lld want=%lld/%lld/%lld/%lld/%lld %s\n", name, (long long)slabs,
           (long long)groups, (long long)steps, (long long)segs, (long long)plan.max_rows, (long long)want_slabs, (long long)want_groups,
           (long long)want_steps, (long long)want_segs, (long long)want_max_rows, ok ? "ok" : "MISMATCH");
    g_fails += !ok;
}

int main()
{
    const size_t big = size_t(512) << 20;
    const int64_t chunk_rows = (int64_t)F1X_CHUNK_WORDS * 64, step_rows = F1X_STEP_ROWS;
    const size_t step_bytes_64 = (size_t)f1x_step_bytes(64);         // planes of one step at 64 padded columns
    const int ppms[4] = {0, 1000, 400000, 1000000};
    // ---- the plan alone (the window sets of par_host_driver; every touched word is a segment here)
    plan_case("bit0", cuts(200, {64}), big, 64, 1, 1, 1, 4, 200);                       // a boundary at bit 0 of word 1: no word is split
    plan_case("bit63", cuts(200, {63}), big, 64, 1, 1, 1, 5, 200);                      // ... at bit 63 of word 0: that word gives two segments
    plan_case("many-in-a-word", cuts(200, {70, 71, 75, 100}), big, 64, 1, 1, 1, 8, 200);      // four boundaries inside word 1: five segments of it
    plan_case("empty-windows", cuts(200, {0, 0, 90, 90, 90, 200, 200}), big, 64, 1, 1, 1, 5, 200);      // first, in the middle, last
    plan_case("long-window", cuts(2 * chunk_rows + 100, {50, 50 + chunk_rows + 1}), big, 64, 1, 3, 1 + 9 + 9, 2 * (chunk_rows / 64) + 2 + 2, 2 * chunk_rows + 100);
    plan_case("over-budget", cuts(5000, {100, 4200}), 1, 64, 3, 3, 1 + 5 + 1, 2 + 65 + 13, 4100);      // a window of 4100 rows, a budget below one step
    plan_case("three-slabs", every(6 * step_rows, step_rows), 2 * step_bytes_64, 64, 3, 3, 6, 6 * 16, 2 * step_rows);
    plan_case("rows-own", every_row(130), big, 64, 1, 1, 1, 130, 130);
    // ---- kernels
    int k = 0;
    for (int64_t acc : {1, 2, 31, 32, 33, 65})
        for (int64_t rows : {1, 63, 64, 65, 1025}) {
            const Layout lay = (Layout)(k % 3);
            const int ppm = ppms[k % 4], run = 1 + k % 3;
            switch (k++ % 5) {
            case 0: run_case("one-window", lay, rows + 3, acc, 0, 0, one_window(rows), 1, ppm, run, big); break;
            case 1: run_case("rows-own", lay, rows + 3, acc, 0, 0, every_row(rows), 1, ppm, run, big); break;
            case 2: run_case("cuts-63-64-65", lay, rows + 3, acc, 0, 0, cuts(rows, {63, 64, 65}), 2, ppm, run, big); break;
            case 3: run_case("empty-windows", lay, rows + 3, acc, 0, 0, cuts(rows, {0, 0, rows / 2, rows / 2, rows, rows}), 1, ppm, run, big); break;
            default: run_case("windows-of-7", lay, rows + 3, acc, 0, 0, every(rows, 7), 3, ppm, run, big); break;
            }
        }
    // every window set at every row count, on few accessions
    for (int64_t rows : {1, 63, 64, 65, 1025}) {
        run_case("one-window", (Layout)(k++ % 3), rows + 3, 2, 0, 0, one_window(rows), 1, 400000, 1, big);
        run_case("rows-own", (Layout)(k++ % 3), rows + 3, 2, 0, 0, every_row(rows), 1, 0, 2, big);
        run_case("cuts-63-64-65", (Layout)(k++ % 3), rows + 3, 33, 0, 0, cuts(rows, {63, 64, 65}), 1, 400000, 1, big);
        run_case("empty-windows", (Layout)(k++ % 3), rows + 3, 2, 0, 0, cuts(rows, {0, 0, rows / 2, rows / 2, rows, rows}), 1, 1000000, 1, big);
    }
    // one window across an LDS step, in every layout; windows that start and end inside a step's words
    run_case("across-step", INT8, step_rows + 205, 33, 0, 0, cuts(step_rows + 200, {step_rows - 100, step_rows + 100}), 1, 400000, 1, big);
    run_case("across-step", PACKED, step_rows + 205, 65, 0, 0, cuts(step_rows + 200, {step_rows - 1, step_rows + 1}), 2, 1000000, 2, big);
    run_case("across-step", SPLIT, step_rows + 205, 2, 0, 0, one_window(step_rows + 1), 1, 500000, 1, big);
    // one window longer than a chunk at 33 accessions (a group of its own with more steps), between short ones
    run_case("long-window", INT8, chunk_rows + 1300, 33, 0, 0, cuts(chunk_rows + 1290, {70, chunk_rows + 1100}), 1, 450000, 1, big, 0, 3);
    run_case("long-window", SPLIT, chunk_rows + 5, 33, 0, 0, one_window(chunk_rows + 1), 1, 450000, 1, big);
    // 31 / 32 / 33 / 65 windows of 7 rows: the bit words fill exactly and spill by one
    for (int64_t wins : {31, 32, 33, 65})
        run_case("bit-words", (Layout)(k++ % 3), 7 * wins + 3, 33, 0, 0, every(7 * wins, 7), 2, 400000, 2, big);
    // a group boundary inside a bit word: windows of 3000 rows go two to a group, so three groups OR into bit word 0
    run_case("groups-in-a-bit-word", PACKED, 15005, 33, 0, 0, every(15000, 3000), 1, 480000, 1, big, 1, 3);
    // two and three slabs of whole windows: windows of 700 rows, a budget of two steps (two windows) resp. one step (one window) per slab
    run_case("two-slabs", INT8, 2805, 33, 0, 0, every(2800, 700), 1, 450000, 1, 2 * step_bytes_64, 2);
    run_case("three-slabs", PACKED, 2105, 65, 0, 0, every(2100, 700), 5, 450000, 2, (size_t)f1x_step_bytes(128), 3);
    run_case("three-slabs-window-over-budget", SPLIT, 3305, 33, 0, 0, cuts(3300, {100, 2300}), 1, 1000000, 1, 1, 3);
    // column and row lists with repeats; the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28)
    run_case("lists", INT8, 300, 70, 1, 1, every(200, 33), 3, 400000, 1, big);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, cuts(129, {64, 100}), 1, 0, 1, big);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, every(129, 10), 5, 300000, 2, big);
    run_case("list-three-slabs", INT8, 500, 33, 1, 1, every(2100, 700), 1, 450000, 1, step_bytes_64, 3);
    run_case("split-wide", SPLIT, 65, 1135, 0, 0, cuts(65, {20, 21}), 1, 300000, 1, big);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
