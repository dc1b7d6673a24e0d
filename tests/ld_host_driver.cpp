// The kernel source of csrc/snpm_k_ld.hpp compiled for the host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header,
// tests/host_kernel/harness.hpp runs it) with its launch geometry: every block of k_ld_planes by 256 and of k_ld_band by 1024 real
// threads with a barrier for __syncthreads.  Built with -fsanitize=address,undefined by tests/test_ld_cpu.py and run as a child
// process: the panel, the row list of a slab with its halo, the membership words, the planes and the slab's cells are heap blocks of
// exactly the size the library would use, the pad bytes of the rows hold arbitrary values and the workspaces start with stale
// contents; the slab plan is the library's own (ld_slab_rows).  Every count is compared with a brute-force count over the columns,
// every r2 bit with the formula written out here.  Prints "case ... ok" per case and "done fails=0".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "snpm_k_common.hpp"
#include "snpm_k_site.hpp"
#include "snpm_k_ld.hpp"

#include "harness.hpp"

// the pitches of the library (TIGHT: no wide loads unless n_acc is a multiple of 16), anything in the pad bytes
static const PanelStyle kStyle = {true, true, false};

static int g_fails = 0;

static double want_r2(const int64_t *c, int64_t va, int64_t vh, int64_t min_n)
{
    const int64_t n = c[0], sx = va * c[1] + vh * c[2], sxx = va * va * c[1] + vh * vh * c[2], sy = va * c[3] + vh * c[4];
    const int64_t syy = va * va * c[3] + vh * vh * c[4], sxy = va * va * c[5] + va * vh * (c[6] + c[7]) + vh * vh * c[8];
    const int64_t num = n * sxy - sx * sy, dx = n * sxx - sx * sx, dy = n * syy - sy * sy;
    if (n < min_n || dx == 0 || dy == 0) return NAN;
    const volatile double nn = (double)num * (double)num, dd = (double)dx * (double)dy;     // (volatile: two roundings, then the third)
    return nn / dd;
}

// the launches of snpm_panel_ld_band, with `ws_bytes` as the workspace budget.  subset: every third column is left out (and the
// list is not sorted); use_rows: a row list, unsorted, with a repeat; outs: 1 = counts, 2 = r2, 3 = both
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int64_t n_rows, int64_t band, int subset, int use_rows, int outs,
                     size_t ws_bytes, int v_alt = 2, int v_het = 1, int min_n = 2)
{
    Panel p = make_panel(lay, n_snp, n_acc, kStyle);
    const int64_t words = (n_acc + 31) / 32;
    std::vector<int64_t> cols;
    for (int64_t c = n_acc - 1; c >= 0; --c)
        if (!subset || c % 3 != 1) cols.push_back(c);
    std::vector<uint32_t> plain((size_t)words, 0u);
    for (int64_t c : cols) plain[(size_t)(c >> 5)] |= 1u << (c & 31);
    uint32_t *member = (uint32_t *)exact_block((size_t)words * sizeof(uint32_t));
    for (int64_t w = 0; w < words; ++w) member[w] = site_member_word(plain.data(), words, p.packed, 0, (int)w, 0);
    int64_t row0 = 0, *rows = nullptr;
    if (use_rows) {
        rows = (int64_t *)exact_block((size_t)n_rows * sizeof(int64_t));
        for (int64_t r = 0; r < n_rows; ++r) rows[r] = (int64_t)(rnd() % n_snp);
        if (n_rows > 2) rows[n_rows - 1] = rows[0];
    } else {
        row0 = n_snp - n_rows;              // the range ends with the panel
    }
    const size_t cells = (size_t)(n_rows * band);
    int32_t *counts = (outs & 1) ? (int32_t *)exact_block(cells * 36) : nullptr;
    double *r2 = (outs & 2) ? (double *)exact_block(cells * 8) : nullptr;
    if (counts) memset(counts, 0x5A, cells * 36);
    if (r2) memset(r2, 0x5A, cells * 8);
    const bool wide = site_wide_rows(p.d, p.pitch, p.desc);
    int slabs = 0;
    int64_t slab_rows = 0;
    if (n_rows > 0) {
        slab_rows = ld_slab_rows(ws_bytes, words, band, n_rows);
        const int64_t plane_rows = std::min(slab_rows + band, n_rows);
        const size_t plane_bytes = (size_t)(plane_rows * 3 * words) * 4, slab_cells = (size_t)(slab_rows * band);
        uint32_t *planes = (uint32_t *)exact_block(plane_bytes);
        int32_t *ws_c = counts ? (int32_t *)exact_block(slab_cells * 36) : nullptr;
        double *ws_r = r2 ? (double *)exact_block(slab_cells * 8) : nullptr;
        memset(planes, 0xA5, plane_bytes);                            // stale contents
        if (ws_c) memset(ws_c, 0xA5, slab_cells * 36);
        if (ws_r) memset(ws_r, 0xA5, slab_cells * 8);
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0), n_plane = std::min(n_valid + band, n_rows - s0);
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab with its halo, as in the library
            int64_t *slab_list = nullptr;
            if (rows) {
                slab_list = (int64_t *)exact_block((size_t)n_plane * sizeof(int64_t));
                memcpy(slab_list, rows + s0, (size_t)n_plane * sizeof(int64_t));
            }
            const int64_t blocks = (n_plane * words + LD_PLANE_THREADS - 1) / LD_PLANE_THREADS;
            launch(LD_PLANE_THREADS, (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, 2)), 1, [&] {      // two blocks: the stride loop runs
                if (p.packed) {
                    if (wide) k_ld_planes<true, true>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_plane, member, (int)words, planes);
                    else k_ld_planes<true, false>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_plane, member, (int)words, planes);
                } else {
                    if (wide) k_ld_planes<false, true>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_plane, member, (int)words, planes);
                    else k_ld_planes<false, false>(p.d, p.pitch, p.desc, n_acc, slab_list, first, n_plane, member, (int)words, planes);
                }
            });
            launch(LD_THREADS, (unsigned)((n_valid + LD_T - 1) / LD_T), (unsigned)((band + LD_D - 1) / LD_D),
                   [&] { k_ld_band(planes, (int)words, n_plane, n_valid, band, v_alt, v_het, min_n, ws_c, ws_r); });
            if (counts) memcpy(counts + s0 * band * 9, ws_c, (size_t)(n_valid * band) * 36);
            if (r2) memcpy(r2 + s0 * band, ws_r, (size_t)(n_valid * band) * 8);
            free(slab_list);
        }
        free(planes); free(ws_c); free(ws_r);
    }
    long bad = 0;
    for (int64_t k = 0; k < n_rows; ++k)
        for (int64_t d = 1; d <= band; ++d) {
            int64_t want[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (k + d < n_rows) {
                const int64_t pk = rows ? rows[k] : row0 + k, pj = rows ? rows[k + d] : row0 + k + d;
                for (int64_t c : cols) {
                    const int x = p.calls[(size_t)(pk * n_acc + c)], y = p.calls[(size_t)(pj * n_acc + c)];
                    const bool mx = x >= 0 && x <= 2, my = y >= 0 && y <= 2;
                    want[0] += mx && my; want[1] += x == 1 && my; want[2] += x == 2 && my; want[3] += y == 1 && mx; want[4] += y == 2 && mx;
                    want[5] += x == 1 && y == 1; want[6] += x == 1 && y == 2; want[7] += x == 2 && y == 1; want[8] += x == 2 && y == 2;
                }
            }
            const int64_t cell = k * band + d - 1;
            for (int q = 0; q < 9 && counts; ++q) bad += counts[cell * 9 + q] != want[q];
            if (r2) {
                const double w = want_r2(want, v_alt, v_het, min_n), g = r2[cell];
                bad += std::isnan(w) ? !std::isnan(g) : (memcmp(&w, &g, 8) != 0 || g > 1.0);
            }
        }
    printf("case %s layout=%d acc=%lld rows=%lld band=%lld subset=%d list=%d outs=%d wide=%d slabs=%d slab_rows=%lld %s\n", name, (int)lay, (long long)n_acc,
           (long long)n_rows, (long long)band, subset, use_rows, outs, (int)wide, slabs, (long long)slab_rows, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(counts); free(r2); free(rows); free(member); free(p.d);
}

int main()
{
    const size_t big = size_t(256) << 20;
    const int64_t bands[5] = {1, 2, 63, 64, 65};
    int k = 0;
    // every width x every row count, the band and the layout taking turns (rows: 0 / 1 / 2 / band / band + 1 / 63 / 64 / 65)
    for (int64_t acc : {1, 2, 31, 32, 33, 63, 64, 65, 130, 1135})
        for (int which = 0; which < 8; ++which) {
            const int64_t band = bands[k % 5], rows = which == 3 ? band : which == 4 ? band + 1 : which < 3 ? which : 58 + which;
            run_case("small", (Layout)(k % 3), rows + 3, acc, rows, band, k % 4 == 1, 0, 1 + k % 3, big);
            ++k;
        }
    // every band in every layout at the width of the 1001-Genomes panel (split: 256 + 32 bytes per row)
    for (int b = 0; b < 5; ++b)
        for (int lay = 0; lay < 3; ++lay) run_case("1135", (Layout)lay, 70, 1135, 66, bands[b], b == 2, 0, 3, big);
    // rows of a pitch that takes the byte loads; more than one column chunk (24 words = 768 columns); the widest panel
    run_case("tight", TIGHT, 40, 33, 37, 2, 1, 0, 3, big);
    run_case("tight-1135", TIGHT, 20, 1135, 20, 5, 0, 1, 3, big);
    run_case("two-chunks", INT8, 12, 800, 12, 3, 1, 0, 3, big);
    run_case("two-chunks-split", SPLIT, 70, 1601, 66, 65, 0, 0, 3, big);
    run_case("widest", PACKED, 6, 16384, 6, 2, 1, 0, 3, big);
    run_case("widest-int8", INT8, 5, 16384, 5, 1, 0, 0, 3, big);
    // a row list, unsorted, with a repeat; other genotype values and a higher minimum
    run_case("list", INT8, 300, 130, 100, 7, 0, 1, 3, big);
    run_case("list-split", SPLIT, 90, 130, 70, 64, 1, 1, 3, big);
    run_case("values", PACKED, 50, 65, 50, 3, 0, 0, 3, big, 1, 2, 40);
    run_case("values-0-3", INT8, 50, 33, 50, 3, 0, 0, 3, big, 0, 3, 1);
    // two and three slabs (the budget holds 64 rows): the halo crosses every edge, the last slab is shorter than the band
    run_case("two-slabs", PACKED, 120, 65, 100, 50, 0, 0, 3, 1);
    run_case("three-slabs", INT8, 140, 33, 130, 65, 1, 0, 3, 1);
    run_case("list-three-slabs", SPLIT, 50, 130, 131, 5, 0, 1, 3, 1);
    run_case("list-two-slabs-r2", INT8, 40, 7, 70, 64, 0, 1, 2, 1);
    // the arithmetic of the plan (budget, words, band, rows), for engine.ld_slab_rows to agree with
    printf("case plan %lld %lld %lld %lld ok\n", (long long)ld_slab_rows(size_t(1) << 20, 512, 65, 200), (long long)ld_slab_rows(size_t(256) << 20, 36, 50, 11000000),
           (long long)ld_slab_rows(size_t(1) << 20, 36, 4096, 200), (long long)ld_slab_rows(1, 1, 1, 10));
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
