// The kernel source of csrc/snpm_k_mix.hpp (and k_win_planes of csrc/snpm_k_win.hpp, which it is launched behind) compiled for the
// host (tests/host_kernel/hip/hip_runtime.h stands in for the HIP header, tests/host_kernel/harness.hpp runs it) with its launch
// geometry: every block by 256 real threads with a barrier for __syncthreads.  Built with -fsanitize=address,undefined by
// tests/test_mixture_cpu.py and run as a child process: the panel, the row and column lists, the read counts, the bit slices, the
// planes and the table are heap blocks of exactly the size the library would use, the pad bytes of the rows hold arbitrary values and
// the planes start with stale contents; the slab plan, the choice of BITS and the bit slices are the library's own (mix_slab_steps,
// mix_bits_of, mix_fill_masks).  Every sum is compared with a brute-force sum.  Prints "case ... ok" per case and "done fails=0";
// the "case masks" lines carry the words of mix_fill_masks for counts the test forms again.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "snpm_k_common.hpp"
#include "snpm_k_kin.hpp"
#include "snpm_k_win.hpp"
#include "snpm_k_mix.hpp"

#include "harness.hpp"

// rows of exactly their bytes, anything in the pad bytes
static const PanelStyle kStyle = {false, true, false};

static int g_fails = 0;

// the launches of snpm_panel_mix_counts, with `ws_bytes` as the workspace budget; counts 0 .. max_count, the largest present
static void run_case(const char *name, Layout lay, int64_t n_snp, int64_t n_acc, int use_cols, int use_rows, int64_t n_rows, int max_count, size_t ws_bytes)
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
    uint8_t *alt = (uint8_t *)exact_block((size_t)n_rows), *ref = (uint8_t *)exact_block((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) {
        alt[r] = (uint8_t)(rnd() % 4 == 0 ? 0 : rnd() % (uint32_t)(max_count + 1));
        ref[r] = (uint8_t)(rnd() % 4 == 0 ? 0 : rnd() % (uint32_t)(max_count + 1));
    }
    const uint32_t which = rnd() & 1, at = rnd() % (uint32_t)n_rows;
    (which ? alt : ref)[at] = (uint8_t)max_count;
    int seen = 0;
    for (int64_t r = 0; r < n_rows; ++r) seen = std::max(seen, (int)std::max(alt[r], ref[r]));
    const int bits = mix_bits_of(seen);
    const size_t cells = (size_t)(ncols * ncols);
    int32_t *out = (int32_t *)calloc(8 * cells, sizeof(int32_t));
    int slabs = 0;
    {
        const int64_t cols_pad = (ncols + MIX_PL_COLS - 1) / MIX_PL_COLS * MIX_PL_COLS;
        const int n_tiles = (int)((ncols + MIX_TILE - 1) / MIX_TILE);
        const int64_t slab_steps = mix_slab_steps(ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * MIX_STEP_ROWS;
        const size_t plane_bytes = (size_t)(slab_steps * mix_step_bytes(cols_pad));
        unsigned long long *planes = (unsigned long long *)exact_block(plane_bytes);
        memset(planes, 0xA5, plane_bytes);                            // stale contents
        const int64_t all_steps = (n_rows + MIX_STEP_ROWS - 1) / MIX_STEP_ROWS, mw = mix_mask_words(bits);
        unsigned long long *masks = (unsigned long long *)exact_block((size_t)(all_steps * mw) * sizeof(unsigned long long));
        memset(masks, 0x5A, (size_t)(all_steps * mw) * sizeof(unsigned long long));
        mix_fill_masks(alt, ref, n_rows, bits, masks);
        for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows, ++slabs) {
            const int64_t n_valid = std::min(slab_rows, n_rows - s0);
            const int64_t W = (n_valid + MIX_STEP_ROWS - 1) / MIX_STEP_ROWS * MIX_STEP_WORDS;
            const int64_t first = rows ? 0 : row0 + s0;              // a row list travels slab by slab, as in the library
            const int64_t *slab_list = nullptr;
            if (rows) {
                int64_t *copy = (int64_t *)exact_block((size_t)n_valid * sizeof(int64_t));
                memcpy(copy, rows + s0, (size_t)n_valid * sizeof(int64_t));
                slab_list = copy;
            }
            launch(WN_THREADS, (unsigned)W, (unsigned)(cols_pad / MIX_PL_COLS), [&] {
                k_win_planes(p.d, p.pitch, p.desc, slab_list, first, n_valid, cols, ncols, planes, cols_pad, W);
            });
            const unsigned long long *slab_masks = masks + s0 / MIX_STEP_ROWS * mw;
            launch(MIX_THREADS, (unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + MIX_CHUNK_WORDS - 1) / MIX_CHUNK_WORDS), [&] {
                if (bits == 2) k_mix_count<2>(planes, cols_pad, W, slab_masks, (int)ncols, n_tiles, out);
                else if (bits == 4) k_mix_count<4>(planes, cols_pad, W, slab_masks, (int)ncols, n_tiles, out);
                else k_mix_count<8>(planes, cols_pad, W, slab_masks, (int)ncols, n_tiles, out);
            });
            free((void *)slab_list);
        }
        free(masks);
        free(planes);
    }
    // brute force
    long bad = 0;
    std::vector<int8_t> col_a((size_t)n_rows), col_b((size_t)n_rows);
    for (int64_t a = 0; a < ncols; ++a) {
        const int64_t ca = cols ? cols[a] : a;
        for (int64_t r = 0; r < n_rows; ++r) col_a[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + ca)];
        for (int64_t b = 0; b < ncols; ++b) {
            const int64_t cb = cols ? cols[b] : b;
            for (int64_t r = 0; r < n_rows; ++r) col_b[(size_t)r] = p.calls[(size_t)((rows ? rows[r] : row0 + r) * n_acc + cb)];
            int32_t want[2][2][2] = {};
            for (int64_t r = 0; r < n_rows; ++r) {
                const int x = col_a[(size_t)r], y = col_b[(size_t)r];
                if ((x != 0 && x != 1) || (y != 0 && y != 1)) continue;
                want[0][x][y] += alt[r];
                want[1][x][y] += ref[r];
            }
            for (int w = 0; w < 2; ++w)
                for (int x = 0; x < 2; ++x)
                    for (int y = 0; y < 2; ++y) bad += out[((size_t)((w * 2 + x) * 2 + y)) * cells + (size_t)(a * ncols + b)] != want[w][x][y];
        }
    }
    printf("case %s layout=%d acc=%lld cols=%lld rows=%lld max=%d bits=%d slabs=%d %s\n", name, (int)lay, (long long)n_acc, (long long)ncols,
           (long long)n_rows, seen, bits, slabs, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(out); free(alt); free(ref); free(rows); free(cols); free(p.d);
}

static void plan_case(const char *name, int64_t got, int64_t want)
{
    printf("case %s got=%lld want=%lld %s\n", name, (long long)got, (long long)want, got == want ? "ok" : "MISMATCH");
    g_fails += got != want;
}

// the words of mix_fill_masks for alt[k] = (7 k + 3) mod 2^bits, ref[k] = (13 k + 5) mod 2^bits, in hex: the test forms them again
static void masks_case(int bits, int64_t n_rows)
{
    uint8_t *alt = (uint8_t *)exact_block((size_t)n_rows), *ref = (uint8_t *)exact_block((size_t)n_rows);
    for (int64_t k = 0; k < n_rows; ++k) {
        alt[k] = (uint8_t)((7 * k + 3) % (1 << bits));
        ref[k] = (uint8_t)((13 * k + 5) % (1 << bits));
    }
    const int64_t words = (n_rows + MIX_STEP_ROWS - 1) / MIX_STEP_ROWS * mix_mask_words(bits);
    unsigned long long *masks = (unsigned long long *)exact_block((size_t)words * sizeof(unsigned long long));
    memset(masks, 0x5A, (size_t)words * sizeof(unsigned long long));
    mix_fill_masks(alt, ref, n_rows, bits, masks);
    printf("case masks bits=%d rows=%lld step_words=%d words=", bits, (long long)n_rows, MIX_STEP_WORDS);
    for (int64_t i = 0; i < words; ++i) printf("%016llx", masks[i]);
    printf(" ok\n");
    free(masks); free(alt); free(ref);
}

int main()
{
    const size_t big = size_t(512) << 20;
    const int64_t chunk_rows = (int64_t)MIX_CHUNK_WORDS * 64, step_rows = MIX_STEP_ROWS;
    const int maxes[5] = {3, 4, 15, 16, 255};
    int k = 0;
    for (int64_t acc : {1, 2, 31, 32, 33, 65, 130})
        for (int64_t rows : {1, 63, 64, 65}) {
            const Layout lay = (Layout)(k % 3);
            run_case("small", lay, rows + 3, acc, 0, 0, rows, maxes[k % 5], big);
            ++k;
        }
    // one row past an LDS step and past a chunk, in every layout and at every BITS
    run_case("step+1", INT8, step_rows + 5, 33, 0, 0, step_rows + 1, 3, big);
    run_case("step+1", PACKED, step_rows + 5, 65, 0, 0, step_rows + 1, 15, big);
    run_case("step+1", SPLIT, step_rows + 5, 2, 0, 0, step_rows + 1, 255, big);
    run_case("chunk+1", INT8, chunk_rows + 5, 2, 0, 0, chunk_rows + 1, 255, big);
    run_case("chunk+1", PACKED, chunk_rows + 5, 33, 0, 0, chunk_rows + 1, 3, big);
    run_case("chunk+1", SPLIT, chunk_rows + 5, 33, 0, 0, chunk_rows + 1, 15, big);
    // a tile, a step and a chunk crossed at once, at each BITS
    for (int m : {3, 15, 255}) run_case("tile-step-chunk", INT8, chunk_rows + step_rows + 9, 33, 0, 0, chunk_rows + step_rows + 1, m, big);
    // two slabs: one chunk per slab (the budget holds one chunk of the 64 padded columns), and slabs below a chunk (one LDS step each)
    run_case("two-slabs", INT8, chunk_rows + 1100, 33, 0, 0, chunk_rows + 1030, 15, (size_t)(4 * 64 * MIX_CHUNK_WORDS * 8));
    run_case("two-short-slabs", PACKED, 1100, 65, 0, 0, 1030, 255, 1);
    run_case("three-short-slabs", SPLIT, 2200, 33, 0, 0, 2100, 3, 1);
    // column and row lists
    run_case("lists", INT8, 300, 70, 1, 1, 200, 15, big);
    run_case("lists-packed", PACKED, 90, 130, 1, 1, 129, 255, big);
    run_case("lists-split", SPLIT, 90, 130, 1, 1, 129, 3, big);
    run_case("list-three-slabs", INT8, 500, 33, 1, 1, 2100, 16, 1);
    // the plan alone: 65535 chunks (grid.y of k_mix_count) of 8 steps bound a slab however large the budget; a budget below one step
    // takes one; the choice of BITS at its edges
    plan_case("plan-grid-cap", mix_slab_steps(SIZE_MAX, 64, INT32_MAX), 65535 * (MIX_CHUNK_WORDS / MIX_STEP_WORDS));
    plan_case("plan-one-step", mix_slab_steps(1, 64, INT32_MAX), 1);
    for (int m : {0, 3, 4, 15, 16, 255}) plan_case("plan-bits", mix_bits_of(m), m <= 3 ? 2 : m <= 15 ? 4 : 8);
    masks_case(2, 1);
    masks_case(4, step_rows + 6);
    masks_case(8, step_rows - 1);
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
