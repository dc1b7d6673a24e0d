// The kernel source of csrc/snpm_k_mos.hpp (and k_win_planes of csrc/snpm_k_win.hpp, which it is launched behind) compiled for the
// host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header, tests/host_kernel/harness.hpp runs it) with its launch
// geometry: every block by its real threads with a barrier for __syncthreads, the ballots of a wave through its 64
// threads.  Built with -fsanitize=address,undefined by tests/test_mosaic_host_cpu.py and run as a child process: the panel, the row
// and column lists, the class words, the chain table, the planes, the sw words, j and the results are heap blocks of exactly the size
// the library would use, the pad bytes of the rows hold arbitrary values and the workspaces start with stale contents; the plan
// (slabs of whole chains, groups of samples) is the library's own (mos_slab).  Every state, chain cost and column cost is compared
// with a per-row transcription of the model.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"
#include "snpm_k_mos.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;
typedef std::vector<int64_t> Offsets;

static Offsets one_chain(int64_t n) { return {0, n}; }
static Offsets cuts(int64_t n, std::initializer_list<int64_t> at)      // boundaries at the listed rows, as far as they lie inside
{
    Offsets o{0};
    for (int64_t c : at) o.push_back(std::max<int64_t>(0, std::min(c, n)));
    o.push_back(n);
    std::sort(o.begin(), o.end());
    return o;
}
static Offsets every(int64_t n, int64_t len)
{
    Offsets o;
    for (int64_t k = 0; k < n; k += len) o.push_back(k);
    o.push_back(n);
    return o;
}

template <int NW, int T>
static void launch_fwd(int nb, unsigned gx, unsigned gy, const unsigned long long *planes, int64_t cols_pad, int64_t W, const unsigned long long *cls,
                       const int64_t *chains, int ncols, const uint32_t *cb, int32_t S, unsigned long long *sw, int64_t sw_words, int32_t *jarr,
                       int64_t n_rows, int32_t *chain_cost, int32_t *col_cost)
{
    launch(NW * WAVE, gx, gy, [&] {
        if (nb == 2)
            k_mos_fwd<NW, T, 2>(planes, cols_pad, W, cls, chains, ncols, cb[0], cb[1], cb[2], cb[3], S, sw, sw_words, jarr, n_rows, chain_cost, col_cost);
        else
            k_mos_fwd<NW, T, 4>(planes, cols_pad, W, cls, chains, ncols, cb[0], cb[1], cb[2], cb[3], S, sw, sw_words, jarr, n_rows, chain_cost, col_cost);
    });
}

// the launches of snpm_panel_mosaic, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, const Offsets &off, int n_samples,
                     int32_t S, int table, size_t ws_bytes, int want_slabs = 0, int want_groups = 0)
{
    const int64_t n_rows = off.back(), n_chain = (int64_t)off.size() - 1;
    Panel p = make_panel(lay, n_snp, n_acc, kStyle);
    int64_t ncols = n_acc, row0 = 0;
    int32_t *cols = nullptr;
    int64_t *rows = nullptr;
    if (use_cols) {                         // shuffled, with repeats
        ncols = n_acc + 2;
        cols = (int32_t *)exact_block((size_t)ncols * sizeof(int32_t));
        for (int64_t a = 0; a < ncols; ++a) cols[a] = (int32_t)(rnd() % n_acc);
        cols[ncols - 1] = cols[0];
    }
    if (use_rows) {                         // unsorted, with repeats
        rows = (int64_t *)exact_block((size_t)n_rows * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = (int64_t)(rnd() % n_snp);
        if (n_rows > 1) rows[n_rows - 1] = rows[0];
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    // the samples: copies of a column in stretches with a few flipped calls, so that paths switch; the last sample random
    uint8_t *cls = (uint8_t *)exact_block((size_t)(n_samples * n_rows));
    for (int s = 0; s < n_samples; ++s) {
        int64_t src = (int64_t)(rnd() % ncols);
        for (int64_t r = 0; r < n_rows; ++r) {
            if (rnd() % 40 == 0) src = (int64_t)(rnd() % ncols);
            const int v = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + (cols ? cols[src] : src))];
            const uint32_t u = rnd() % 100;
            cls[s * n_rows + r] = (uint8_t)(u < 5 ? 0xFF : (u < 10 || v < 0 || v > 2 || s == n_samples - 1) ? rnd() % 3 : v);
        }
    }
    uint8_t cost[12];
    for (int i = 0; i < 12; ++i) {
        const int c = i / 4, d = i % 4;
        switch (table) {
        case 0: cost[i] = (uint8_t)(d == 3 ? 2 : c == d ? 0 : (c == 2 || d == 2) ? 1 : 2); break;       // the command's default: planes 0 and 1
        case 1: cost[i] = (uint8_t)(rnd() % 16); break;                                                 // anything, zeros off the diagonal among it
        case 2: cost[i] = 0; break;
        default: cost[i] = (uint8_t)(c == d ? 0 : 15); break;
        }
    }
    if (table == 1) cost[1] = 0, cost[6] = 9;
    int64_t *chain_off = (int64_t *)exact_block(off.size() * sizeof(int64_t));
    memcpy(chain_off, off.data(), off.size() * sizeof(int64_t));
    const size_t n_state = (size_t)(n_samples * n_rows), n_cost = (size_t)(n_samples * n_chain), n_cc = n_cost * (size_t)ncols;
    int32_t *state = (int32_t *)exact_block(n_state * 4), *chain_cost = (int32_t *)exact_block(n_cost * 4), *col_cost = (int32_t *)exact_block(n_cc * 4);
    memset(state, 0xA5, n_state * 4);
    memset(chain_cost, 0, n_cost * 4);
    memset(col_cost, 0, n_cc * 4);
    int slabs = 0, groups = 0;
    {
        const int64_t cols_pad = (ncols + WN_PL_COLS - 1) / WN_PL_COLS * WN_PL_COLS;
        uint32_t cb[4];
        const int nb = mos_cost_bits(cost, cb), form = mos_form_of(ncols);
        for (int64_t ch = 0; ch < n_chain;) {
            const MosSlab s = mos_slab(ws_bytes, cols_pad, chain_off, n_chain, ch, n_samples);
            ch = s.ch_hi;
            if (s.n_rows == 0) continue;
            ++slabs;
            const int64_t n_ch = s.ch_hi - s.ch_lo;
            int64_t *chains = (int64_t *)exact_block((size_t)(n_ch * MOS_CHAIN_WORDS) * 8);
            int64_t swb = 0;
            for (int64_t c = 0; c < n_ch; ++c) {
                const int64_t c0 = chain_off[s.ch_lo + c] - s.r0, c1 = chain_off[s.ch_lo + c + 1] - s.r0;
                chains[c * MOS_CHAIN_WORDS] = c0; chains[c * MOS_CHAIN_WORDS + 1] = c1; chains[c * MOS_CHAIN_WORDS + 2] = swb; chains[c * MOS_CHAIN_WORDS + 3] = 0;
                swb += mos_chain_words(c0, c1);
            }
            if (swb != s.sw_words) { ++g_fails; printf("case %s sw words %lld != %lld MISMATCH\n", name, (long long)swb, (long long)s.sw_words); }
            const size_t plane_bytes = (size_t)(4 * cols_pad * s.W * 8);
            unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
            memset(planes, 0xA5, plane_bytes);                        // stale contents
            int64_t *slab_list = nullptr;
            if (rows) {                                               // a row list travels slab by slab, as in the library
                slab_list = (int64_t *)exact_block((size_t)s.n_rows * 8);
                memcpy(slab_list, rows + s.r0, (size_t)s.n_rows * 8);
            }
            launch(WN_THREADS, (unsigned)s.W, (unsigned)(cols_pad / WN_PL_COLS), [&] {
                k_win_planes(p.d, p.pitch, p.desc, slab_list, rows ? 0 : row0 + s.r0, s.n_rows, cols, ncols, planes, cols_pad, s.W);
            });
            for (int64_t g0 = 0; g0 < n_samples; g0 += s.group) {
                ++groups;
                const int64_t g = std::min<int64_t>(s.group, n_samples - g0);
                const size_t sw_bytes = (size_t)(g * s.sw_words * cols_pad * 8), cls_bytes = (size_t)(g * s.W * 3 * 8);
                unsigned long long *sw = (unsigned long long *)exact_block(sw_bytes), *words = (unsigned long long *)exact_block(cls_bytes);
                memset(sw, 0xA5, sw_bytes);
                memset(words, 0, cls_bytes);
                for (int64_t i = 0; i < g; ++i)
                    for (int64_t k = 0; k < s.n_rows; ++k) {
                        const uint8_t c = cls[(g0 + i) * n_rows + s.r0 + k];
                        if (c <= 2) words[(i * s.W + (k >> 6)) * 3 + c] |= 1ull << (k & 63);
                    }
                int32_t *jarr = (int32_t *)exact_block((size_t)(g * s.n_rows) * 4), *d_state = (int32_t *)exact_block((size_t)(g * s.n_rows) * 4);
                int32_t *d_cost = (int32_t *)exact_block((size_t)(g * n_ch) * 4), *d_cc = (int32_t *)exact_block((size_t)(g * n_ch * ncols) * 4);
                memset(jarr, 0xA5, (size_t)(g * s.n_rows) * 4);
                memset(d_state, 0xA5, (size_t)(g * s.n_rows) * 4);
                memset(d_cost, 0, (size_t)(g * n_ch) * 4);
                memset(d_cc, 0, (size_t)(g * n_ch * ncols) * 4);
#define FWD(F) launch_fwd<MOS_FORMS[F].nw, MOS_FORMS[F].t>(nb, (unsigned)n_ch, (unsigned)g, planes, cols_pad, s.W, words, chains, (int)ncols, cb, S, sw, s.sw_words, jarr, s.n_rows, d_cost, d_cc)
                switch (form) {
                case 0: FWD(0); break;
                case 1: FWD(1); break;
                case 2: FWD(2); break;
                default: FWD(3); break;
                }
#undef FWD
                launch(WAVE, (unsigned)n_ch, (unsigned)g, [&] { k_mos_back(sw, s.sw_words, cols_pad, jarr, s.n_rows, chains, d_state); });
                for (int64_t i = 0; i < g; ++i) {
                    memcpy(state + (g0 + i) * n_rows + s.r0, d_state + i * s.n_rows, (size_t)s.n_rows * 4);
                    memcpy(chain_cost + (g0 + i) * n_chain + s.ch_lo, d_cost + i * n_ch, (size_t)n_ch * 4);
                    memcpy(col_cost + ((g0 + i) * n_chain + s.ch_lo) * ncols, d_cc + i * n_ch * ncols, (size_t)(n_ch * ncols) * 4);
                }
                free(d_cc); free(d_cost); free(d_state); free(jarr); free(words); free(sw);
            }
            free(slab_list); free(planes); free(chains);
        }
    }
    // the model, row by row
    long bad = 0;
    std::vector<int32_t> e((size_t)(n_rows * ncols)), V((size_t)ncols), jj((size_t)n_rows), want((size_t)n_rows);
    std::vector<uint8_t> swm((size_t)(n_rows * ncols));
    for (int s = 0; s < n_samples; ++s) {
        for (int64_t r = 0; r < n_rows; ++r)
            for (int64_t a = 0; a < ncols; ++a) {
                const int v = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + (cols ? cols[a] : a))];
                const uint8_t c = cls[s * n_rows + r];
                e[(size_t)(r * ncols + a)] = (c > 2 || v < 0) ? 0 : cost[c * 4 + v];
            }
        for (int64_t c = 0; c < n_chain; ++c) {
            const int64_t c0 = off[(size_t)c], c1 = off[(size_t)c + 1];
            if (c1 <= c0) {
                bad += chain_cost[s * n_chain + c] != 0;
                for (int64_t a = 0; a < ncols; ++a) bad += col_cost[(s * n_chain + c) * ncols + a] != 0;
                continue;
            }
            for (int64_t a = 0; a < ncols; ++a) {
                int32_t sum = 0;
                for (int64_t k = c0; k < c1; ++k) sum += e[(size_t)(k * ncols + a)];
                bad += col_cost[(s * n_chain + c) * ncols + a] != sum;
                V[(size_t)a] = e[(size_t)(c0 * ncols + a)];
            }
            auto lowest = [&](int32_t &B) { int64_t j = 0; for (int64_t a = 1; a < ncols; ++a) if (V[(size_t)a] < V[(size_t)j]) j = a; B = V[(size_t)j]; return (int32_t)j; };
            for (int64_t k = c0 + 1; k < c1; ++k) {
                int32_t B;
                jj[(size_t)(k - 1)] = lowest(B);
                for (int64_t a = 0; a < ncols; ++a) {
                    swm[(size_t)(k * ncols + a)] = V[(size_t)a] > B + S;
                    V[(size_t)a] = std::min(V[(size_t)a], B + S) + e[(size_t)(k * ncols + a)];
                }
            }
            int32_t B;
            int32_t st = lowest(B);
            bad += chain_cost[s * n_chain + c] != B;
            want[(size_t)(c1 - 1)] = st;
            for (int64_t k = c1 - 1; k > c0; --k) {
                if (swm[(size_t)(k * ncols + st)]) st = jj[(size_t)(k - 1)];
                want[(size_t)(k - 1)] = st;
            }
            for (int64_t k = c0; k < c1; ++k) bad += state[s * n_rows + k] != want[(size_t)k];
        }
    }
    const bool plan_ok = (want_slabs == 0 || slabs == want_slabs) && (want_groups == 0 || groups == want_groups);
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld chains=%lld samples=%d S=%d table=%d slabs=%d groups=%d %s\n", name, (int)lay, (long long)n_acc,
           (long long)ncols, (long long)n_rows, (long long)n_chain, n_samples, (int)S, table, slabs, groups, bad || !plan_ok ? "MISMATCH" : "ok");
    g_fails += bad != 0 || !plan_ok;
    free(col_cost); free(chain_cost); free(state); free(chain_off); free(cls); free(rows); free(cols); free(p.d);
}

int main()
{
    const size_t big = size_t(512) << 20;
    int k = 0;
    // every width edge of the forms (64 = one wave, 256 = four waves of one column, 1280 = four waves of five) on few rows
    for (int64_t acc : {1, 2, 63, 64, 65, 130, 255, 256, 257, 1279, 1280, 1281}) {
        const int64_t rows = acc > 1000 ? 70 : 130;
        run_case("widths", (Layout)(k % 3), rows + 3, acc, 0, 0, cuts(rows, {64, 65}), 1, (int32_t)(k % 2 ? 7 : 1), k % 2, big);
        ++k;
    }
    // every row edge, one chain and several
    for (int64_t rows : {1, 2, 63, 64, 65, 1023, 1024, 1025}) {
        run_case("rows-one-chain", (Layout)(k++ % 3), rows + 3, 5, 0, 0, one_chain(rows), 2, 3, 0, big);
        run_case("rows-chains", (Layout)(k++ % 3), rows + 3, 66, 0, 0, cuts(rows, {1, 63, 64, 65, rows - 1}), 1, 7, 1, big);
    }
    // several boundaries inside one word; empty chains first, last and in the middle; chains of one row
    run_case("in-a-word", INT8, 203, 7, 0, 0, cuts(200, {70, 71, 75, 100}), 2, 2, 0, big);
    run_case("empty-chains", PACKED, 203, 7, 0, 0, cuts(200, {0, 0, 90, 90, 90, 200, 200}), 2, 2, 1, big);
    run_case("rows-own", SPLIT, 133, 3, 0, 0, every(130, 1), 1, 1, 0, big);
    // the switch cost at its ends, the tables
    run_case("S-max", INT8, 303, 9, 0, 0, cuts(300, {100}), 2, 1 << 20, 0, big);
    run_case("zero-table", PACKED, 203, 9, 0, 0, cuts(200, {100}), 1, 5, 2, big);
    run_case("table-15", INT8, 203, 9, 0, 0, cuts(200, {100}), 2, 40, 3, big);
    // column and row lists
    run_case("lists", INT8, 300, 70, 1, 1, every(200, 33), 2, 7, 0, big);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, cuts(129, {64, 100}), 1, 1, 1, big);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, every(129, 10), 2, 3, 0, big);
    run_case("split-wide", SPLIT, 65, 1135, 0, 0, cuts(65, {20, 21}), 1, 4, 0, big);
    // slabs of whole chains under a small budget: chains of 700 rows, one per slab; a chain over the budget; samples in groups
    {
        const size_t planes_64 = 32 * 64 * 16, sample_64 = (size_t)mos_sample_bytes(64, 16, 12, 700);
        run_case("three-slabs", INT8, 2105, 33, 0, 0, every(2100, 700), 1, 3, 0, planes_64 + sample_64, 3, 3);
        run_case("groups-of-two", PACKED, 705, 33, 0, 0, one_chain(700), 5, 3, 0, planes_64 + 2 * sample_64 + 8, 1, 3);
        run_case("chain-over-budget", SPLIT, 3305, 33, 1, 1, cuts(3300, {100, 2300}), 3, 2, 1, 1, 3, 9);
    }
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
