// The kernel source of csrc/snpm_k_site.hpp compiled for the host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header,
// tests/host_kernel/harness.hpp runs it) with its launch geometry: every block by 512 real threads with a barrier for __syncthreads,
// the shuffles of a wave through its 64 threads.  Built with -fsanitize=address,undefined by tests/test_sitestats_cpu.py and run as
// a child process: the panel, the row list, the membership words and the slab's counts are heap blocks of exactly the size the
// library would use, the pad bytes of the rows hold arbitrary values and the workspace starts with stale contents; the slab plan is
// the library's own (site_slab_rows).  Every count is compared with a brute-force count.  Prints "case ... ok" per case and
// "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>

#include "snpm_k_common.hpp"
#include "snpm_k_site.hpp"

#include "harness.hpp"

// the pitches of the library (TIGHT: no wide loads unless n_acc is a multiple of 16), anything in the pad bytes
static const PanelStyle kStyle = {true, true, false};

static int g_fails = 0;

// the groups of a case as bitmasks over the panel's columns: 1 = all accessions; 2 = one column, a subset; 3 = a subset, an empty
// group, a subset that overlaps the first; more = subsets with group 5 empty and group 6 of one column
static std::vector<uint32_t> make_groups(int n_groups, int64_t n_acc)
{
    const int64_t nwords = (n_acc + 31) / 32;
    std::vector<uint32_t> m((size_t)(n_groups * nwords), 0u);
    auto set = [&](int g, int64_t c) { m[(size_t)(g * nwords + (c >> 5))] |= 1u << (c & 31); };
    for (int g = 0; g < n_groups; ++g) {
        const bool all = n_groups == 1, empty = (n_groups == 3 && g == 1) || (n_groups > 3 && g == 5);
        const bool one = (n_groups == 2 && g == 0) || (n_groups > 3 && g == 6);
        if (empty) continue;
        if (one) { set(g, (int64_t)(rnd() % n_acc)); continue; }
        for (int64_t c = 0; c < n_acc; ++c)
            if (all || rnd() % 3 != 0) set(g, c);
        if (n_groups == 3 && g == 2) set(g, 0), set(0, 0);          // the first and the last group share column 0 for sure
    }
    return m;
}

// the launches of snpm_panel_site_counts, with `ws_bytes` as the workspace budget
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int n_groups, int use_rows, int64_t n_rows, size_t ws_bytes)
{
    Panel p = make_panel(lay, n_snp, n_acc, kStyle);
    const int64_t nwords = (n_acc + 31) / 32;
    const std::vector<uint32_t> groups = make_groups(n_groups, n_acc);
    uint32_t *member = (uint32_t *)exact_block(groups.size() * sizeof(uint32_t));
    memcpy(member, groups.data(), groups.size() * sizeof(uint32_t));
    int64_t row0 = 0, *rows = nullptr;
    if (use_rows) {                         // unsorted, with repeats
        rows = (int64_t *)exact_block((size_t)n_rows * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = (int64_t)(rnd() % n_snp);
        if (n_rows > 2) rows[n_rows - 1] = rows[0];
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    int32_t *counts = (int32_t *)exact_block((size_t)(n_groups * n_rows) * 16);
    memset(counts, 0x5A, (size_t)(n_groups * n_rows) * 16);
    int lg_s = 0, cpl = 0, slabs = 0;
    if (!site_geometry(n_acc, p.packed, &lg_s, &cpl)) { printf("case %s: panel too wide\n", name); ++g_fails; return; }
    const bool wide = site_wide_rows(p.d, p.pitch, p.desc);
    if (n_rows > 0) {
        const int64_t slab_rows = site_slab_rows(ws_bytes, n_groups, n_rows);
        const size_t out_bytes = (size_t)(n_groups * slab_rows) * 16;
        int32_t *ws = (int32_t *)exact_block(out_bytes);
        memset(ws, 0xA5, out_bytes);                                  // stale contents
        const int rpw = WAVE >> lg_s, waves = SITE_THREADS / WAVE;
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab, as in the library
            int64_t *slab_list = nullptr;
            if (rows) {
                slab_list = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(slab_list, rows + s0, (size_t)n_valid * sizeof(int64_t));
            }
            const int64_t batches = (n_valid + rpw - 1) / rpw;
            const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((batches + waves - 1) / waves, 2));     // two blocks: the stride loop runs
            launch(SITE_THREADS, grid, 1, [&] {
                if (p.packed) {
                    if (wide) k_site_counts<true, true>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                    else k_site_counts<true, false>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                } else {
                    if (wide) k_site_counts<false, true>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                    else k_site_counts<false, false>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_valid, member, n_groups, lg_s, cpl, ws);
                }
            });
            for (int g = 0; g < n_groups; ++g) memcpy(counts + (g * n_rows + s0) * 4, ws + g * n_valid * 4, (size_t)n_valid * 16);
            free(slab_list);
        }
        free(ws);
    }
    long bad = 0;
    for (int g = 0; g < n_groups; ++g)
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t prow = rows ? rows[r] : row0 + r;
            int32_t want[4] = {0, 0, 0, 0};
            for (int64_t c = 0; c < n_acc; ++c) {
                if (!((groups[(size_t)(g * nwords + (c >> 5))] >> (c & 31)) & 1u)) continue;
                const int v = p.calls[(size_t)(prow * n_acc + c)];
                if (v >= 0 && v <= 2) ++want[v];
                want[3] += v >= 0;
            }
            bad += memcmp(want, counts + (g * n_rows + r) * 4, 16) != 0;
        }
    printf("case %s layout=%d acc=%lld groups=%d rows=%lld lanes=%d chunks=%d wide=%d slabs=%d %s\n", name, (int)lay, (long long)n_acc, n_groups,
           (long long)n_rows, 1 << lg_s, cpl, (int)wide, slabs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(counts); free(rows); free(member); free(p.d);
}

int main()
{
    const size_t big = size_t(256) << 20;
    const int group_counts[4] = {1, 2, 3, SNPM_SITE_MAX_GROUPS};
    int k = 0;
    for (int64_t acc : {1, 2, 31, 32, 33, 63, 64, 65, 130, 1135})
        for (int64_t rows : {0, 1, 63, 64, 65}) {
            const Layout lay = (Layout)(k % 3);
            run_case("small", lay, rows + 3, acc, group_counts[(k / 3) % 4], 0, rows, big);
            ++k;
        }
    // the width of the 1001-Genomes panel in every layout (split: 256 + 32 bytes per row), with every group count
    run_case("1135-int8", INT8, 70, 1135, 3, 0, 65, big);
    run_case("1135-packed", PACKED, 70, 1135, SNPM_SITE_MAX_GROUPS, 0, 65, big);
    run_case("1135-split", SPLIT, 70, 1135, 2, 0, 65, big);
    run_case("1135-split-all", SPLIT, 70, 1135, 1, 0, 64, big);
    // rows of a pitch that takes the byte loads, and a whole wave per row (more than 4096 int8 columns)
    run_case("tight", TIGHT, 40, 33, 3, 0, 37, big);
    run_case("tight-1135", TIGHT, 20, 1135, 2, 1, 30, big);
    run_case("whole-wave", INT8, 9, 5000, 3, 0, 9, big);
    run_case("whole-wave-packed", PACKED, 9, 16384, 2, 0, 9, big);
    // a row list with repeats; two slabs (the budget holds 64 rows of the groups), as a range and as a list
    run_case("list", INT8, 300, 130, 3, 1, 200, big);
    run_case("list-split", SPLIT, 90, 130, SNPM_SITE_MAX_GROUPS, 1, 129, big);
    run_case("two-slabs", PACKED, 120, 65, 3, 0, 100, 1);
    run_case("list-two-slabs", INT8, 50, 33, 2, 1, 128, 1);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
