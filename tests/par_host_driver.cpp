// The kernel source of csrc/snpm_k_par.hpp (and k_win_planes of csrc/snpm_k_win.hpp, which it is launched behind) compiled for the
// host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header, tests/host_kernel/harness.hpp runs it) with its launch
// geometry: every block by 256 real threads with a barrier for __syncthreads, the ballots of a wave through its 64 threads.  Built
// with -fsanitize=address,undefined by tests/test_parentsearch_cpu.py and run as a child process: the panel, the row and column
// lists, the classes, the plan's tables, the planes and the results are heap blocks of exactly the size the library would use, the
// pad bytes of the rows hold arbitrary values and the planes start with stale contents; the plan (slabs, groups, segments) is the
// library's own (par_plan) and is checked on its own first: replayed bit by bit against the classes and the windows.  Every count
// is compared with a brute-force count.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"
#include "snpm_k_f1x.hpp"
#include "snpm_k_par.hpp"

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

// the plan replayed: every class bit of every segment is a classed row of the window the stream is in, every classed row of a
// window comes exactly once, a window's last kept segment carries the flag; groups hold whole steps inside the slab's planes
static long replay_plan(const ParPlan &plan, const uint8_t *cls, const Offsets &off)
{
    long bad = 0;
    const int64_t n_win = (int64_t)off.size() - 1;
    int64_t w = 0, seen = 0, want_total = 0;
    auto classed = [&](int64_t win) { int64_t c = 0; for (int64_t r = off[(size_t)win]; r < off[(size_t)win + 1]; ++r) c += cls[r] <= 2; return c; };
    for (int64_t k = 0; k < n_win; ++k) want_total += classed(k);
    int64_t in_window = 0, prev_hi = 0;
    for (const ParSlab &s : plan.slabs) {
        bad += s.w_lo != prev_hi && [&] { for (int64_t k = prev_hi; k < s.w_lo; ++k) if (off[(size_t)k + 1] != off[(size_t)k]) return true; return false; }();
        prev_hi = s.w_hi;
        bad += s.r0 != off[(size_t)s.w_lo] || s.n_rows != off[(size_t)s.w_hi] - s.r0 || s.n_rows <= 0 || s.W != par_words(s.n_rows) || s.W > plan.max_W;
        for (int64_t g = s.g_lo; g < s.g_hi; ++g) {
            const int64_t gw0 = plan.groups[(size_t)(3 * g)], steps = plan.groups[(size_t)(3 * g + 1)], sb = plan.groups[(size_t)(3 * g + 2)];
            bad += gw0 % F1X_STEP_WORDS != 0 || steps < 1 || gw0 + steps * F1X_STEP_WORDS > s.W || sb + steps >= (int64_t)plan.step_off.size();
            for (int64_t st = 0; st < steps; ++st)
                for (int64_t q = plan.step_off[(size_t)(sb + st)]; q < plan.step_off[(size_t)(sb + st + 1)]; ++q) {
                    const unsigned long long *sg = plan.segs.data() + q * PAR_SEG_WORDS;
                    while (w < n_win && (off[(size_t)w + 1] <= s.r0 || classed(w) == 0 || w < s.w_lo)) ++w, in_window = 0;
                    if (w >= s.w_hi) { ++bad; continue; }
                    bad += (sg[0] | sg[1] | sg[2]) == 0 || (sg[0] & sg[1]) || (sg[0] & sg[2]) || (sg[1] & sg[2]) || (sg[3] >> 5);
                    const int64_t word = gw0 + st * F1X_STEP_WORDS + (int64_t)(sg[3] & 15);
                    for (int c = 0; c < 3; ++c)
                        for (int b = 0; b < 64; ++b)
                            if (sg[c] >> b & 1) {
                                const int64_t r = s.r0 + word * 64 + b;
                                bad += r < off[(size_t)w] || r >= off[(size_t)w + 1] || cls[r] != c;
                                ++in_window, ++seen;
                            }
                    if (sg[3] & PAR_SEG_END) {
                        bad += in_window != classed(w);
                        ++w, in_window = 0;
                    }
                }
        }
    }
    bad += seen != want_total || in_window != 0;
    return bad;
}

// the launches of snpm_panel_parent_counts, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, const Offsets &off, int min_sites,
                     size_t ws_bytes, int want_slabs = 0)
{
    const int64_t n_rows = off.back(), n_win = (int64_t)off.size() - 1;
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
    int64_t *win_off = (int64_t *)exact_block(off.size() * sizeof(int64_t));
    memcpy(win_off, off.data(), off.size() * sizeof(int64_t));
    const size_t cells = (size_t)(ncols * ncols);
    int32_t *out = (int32_t *)calloc(4 * cells, sizeof(int32_t));
    long plan_bad = 0;
    int slabs = 0;
    int64_t n_groups = 0, n_segs = 0;
    {
        const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
        const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
        ParPlan plan;
        par_plan(ws_bytes, cols_pad, cls, win_off, n_win, plan);
        plan_bad = replay_plan(plan, cls, off);
        slabs = (int)plan.slabs.size();
        n_groups = (int64_t)plan.groups.size() / PAR_GROUP_WORDS;
        n_segs = (int64_t)plan.segs.size() / PAR_SEG_WORDS;
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
        for (const ParSlab &s : plan.slabs) {
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
                launch(PAR_THREADS, (unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)(s.g_hi - s.g_lo), [&] {
                    k_par_count(planes, cols_pad, s.W, d_groups + s.g_lo * PAR_GROUP_WORDS, d_steps, d_segs, (int)ncols, n_tiles, min_sites, out,
                                out + cells, out + 2 * cells, out + 3 * cells);
                });
            free((void *)slab_list);
        }
        free(d_segs); free(d_steps); free(d_groups); free(planes);
    }
    // brute force, every ordered cell on its own
    long bad = 0, none = 0;
    std::vector<int8_t> col_a((size_t)n_rows), col_b((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) none += cls[r] == 0xFF;
    for (int64_t a = 0; a < ncols; ++a) {
        const int64_t ca = cols ? cols[a] : a;
        for (int64_t r = 0; r < n_rows; ++r) col_a[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + ca)];
        for (int64_t b = 0; b < ncols; ++b) {
            const int64_t cb = cols ? cols[b] : b;
            for (int64_t r = 0; r < n_rows; ++r) col_b[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + cb)];
            int32_t score = 0, ntot = 0, wfirst = 0, whet = 0;
            for (int64_t w = 0; w < n_win; ++w) {
                int32_t n = 0, hA = 0, hB = 0, hF = 0;
                for (int64_t r = off[(size_t)w]; r < off[(size_t)w + 1]; ++r) {
                    const int x = col_a[(size_t)r], y = col_b[(size_t)r], s = cls[r];
                    const int f1 = (x == 0 && y == 0) ? 0 : (x == 1 && y == 1) ? 1 : (x >= 0 && y >= 0 && x != y) ? 2 : -1;
                    if (f1 < 0 || s > 2) continue;
                    ++n;
                    hA += x == s;
                    hB += y == s;
                    hF += f1 == s;
                }
                if (n < min_sites) continue;
                ntot += n;
                if (hF > std::max(hA, hB)) { score += hF; ++whet; }
                else { score += std::max(hA, hB); wfirst += hA > hB || (hA == hB && a <= b); }
            }
            const size_t at = (size_t)(a * ncols + b);
            bad += out[at] != score || out[cells + at] != ntot || out[2 * cells + at] != wfirst || out[3 * cells + at] != whet;
        }
    }
    const bool slabs_ok = want_slabs == 0 || slabs == want_slabs;
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld windows=%lld min=%d noclass=%ld slabs=%d groups=%lld segs=%lld %s\n", name, (int)lay,
           (long long)n_acc, (long long)ncols, (long long)n_rows, (long long)n_win, min_sites, none, slabs, (long long)n_groups, (long long)n_segs,
           bad || plan_bad || !slabs_ok ? "MISMATCH" : "ok");
    g_fails += bad != 0 || plan_bad != 0 || !slabs_ok;
    free(out); free(win_off); free(cls); free(rows); free(cols); free(p.d);
}

// the plan alone, on classes that are all set: slabs, groups, steps and segments of a window set
static void plan_case(const char *name, const Offsets &off, size_t ws_bytes, int64_t cols_pad, int64_t want_slabs, int64_t want_groups, int64_t want_steps,
                      int64_t want_segs, int64_t want_max_rows)
{
    const int64_t n_rows = off.back();
    uint8_t *cls = (uint8_t *)exact_block((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) cls[r] = (uint8_t)(r % 3);
    ParPlan plan;
    par_plan(ws_bytes, cols_pad, cls, off.data(), (int64_t)off.size() - 1, plan);
    const int64_t slabs = (int64_t)plan.slabs.size(), groups = (int64_t)plan.groups.size() / PAR_GROUP_WORDS;
    const int64_t steps = (int64_t)plan.step_off.size() - 1, segs = (int64_t)plan.segs.size() / PAR_SEG_WORDS;
    const bool ok = replay_plan(plan, cls, off) == 0 && slabs == want_slabs && groups == want_groups && steps == want_steps && segs == want_segs &&
                    plan.max_rows == want_max_rows;
    printf("case plan-%s slabs=%lld groups=%lld steps=%lld segs=%lld max_rows=%lld want=%lld/%lld/%lld/%lld/%lld %s\n", name, (long long)slabs,
           (long long)groups, (long long)steps, (long long)segs, (long long)plan.max_rows, (long long)want_slabs, (long long)want_groups,
           (long long)want_steps, (long long)want_segs, (long long)want_max_rows, ok ? "ok" : "MISMATCH");
    g_fails += !ok;
    free(cls);
}

int main()
{
    const size_t big = size_t(512) << 20;
    const int64_t chunk_rows = (int64_t)F1X_CHUNK_WORDS * 64, step_rows = F1X_STEP_ROWS;
    const size_t step_bytes_64 = (size_t)f1x_step_bytes(64);         // planes of one step at 64 padded columns
    // ---- the plan alone
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
            switch (k++ % 5) {
            case 0: run_case("one-window", lay, rows + 3, acc, 0, 0, one_window(rows), 1, big); break;
            case 1: run_case("rows-own", lay, rows + 3, acc, 0, 0, every_row(rows), 1, big); break;
            case 2: run_case("cuts-63-64-65", lay, rows + 3, acc, 0, 0, cuts(rows, {63, 64, 65}), 2, big); break;
            case 3: run_case("empty-windows", lay, rows + 3, acc, 0, 0, cuts(rows, {0, 0, rows / 2, rows / 2, rows, rows}), 1, big); break;
            default: run_case("windows-of-7", lay, rows + 3, acc, 0, 0, every(rows, 7), 5, big); break;
            }
        }
    // every window set at every row count, on few accessions
    for (int64_t rows : {1, 63, 64, 65, 1025}) {
        run_case("one-window", (Layout)(k++ % 3), rows + 3, 2, 0, 0, one_window(rows), 1, big);
        run_case("rows-own", (Layout)(k++ % 3), rows + 3, 2, 0, 0, every_row(rows), 1, big);
        run_case("cuts-63-64-65", (Layout)(k++ % 3), rows + 3, 33, 0, 0, cuts(rows, {63, 64, 65}), 1, big);
        run_case("empty-windows", (Layout)(k++ % 3), rows + 3, 2, 0, 0, cuts(rows, {0, 0, rows / 2, rows / 2, rows, rows}), 1, big);
    }
    // one window across an LDS step, in every layout; windows that start and end inside a step's words
    run_case("across-step", INT8, step_rows + 205, 33, 0, 0, cuts(step_rows + 200, {step_rows - 100, step_rows + 100}), 1, big);
    run_case("across-step", PACKED, step_rows + 205, 65, 0, 0, cuts(step_rows + 200, {step_rows - 1, step_rows + 1}), 5, big);
    run_case("across-step", SPLIT, step_rows + 205, 2, 0, 0, one_window(step_rows + 1), 1, big);
    // one window longer than a chunk at 33 accessions (a group of its own with more steps), between short ones
    run_case("long-window", INT8, chunk_rows + 1300, 33, 0, 0, cuts(chunk_rows + 1290, {70, chunk_rows + 1100}), 1, big);
    run_case("long-window", SPLIT, chunk_rows + 5, 33, 0, 0, one_window(chunk_rows + 1), 1, big);
    // two and three slabs of whole windows: windows of 700 rows, a budget of two steps (two windows) resp. one step (one window) per slab
    run_case("two-slabs", INT8, 2805, 33, 0, 0, every(2800, 700), 1, 2 * step_bytes_64, 2);
    run_case("three-slabs", PACKED, 2105, 65, 0, 0, every(2100, 700), 5, (size_t)f1x_step_bytes(128), 3);
    run_case("three-slabs-window-over-budget", SPLIT, 3305, 33, 0, 0, cuts(3300, {100, 2300}), 1, 1, 3);
    // column and row lists; the width at which the split layout has a main part (1135 accessions: 284 bytes = 256 + 28)
    run_case("lists", INT8, 300, 70, 1, 1, every(200, 33), 3, big);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, cuts(129, {64, 100}), 1, big);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, every(129, 10), 5, big);
    run_case("list-three-slabs", INT8, 500, 33, 1, 1, every(2100, 700), 1, step_bytes_64, 3);
    run_case("split-wide", SPLIT, 65, 1135, 0, 0, cuts(65, {20, 21}), 1, big);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
