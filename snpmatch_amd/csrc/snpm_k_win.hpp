// snpm_k_win.hpp -- panel windows: per genome window, the call counts of every accession column and the agreement counts of listed pairs of columns (Genotype.calculate_heterozygosity_windows / mismatch_between_accs, core/snp_genotype.py:297-345 of the reference).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs pk_off / WAVE of snpm_k_common.hpp and
// kin_code of snpm_k_kin.hpp only, so that tests/win_host_driver.cpp can compile this very text for the host (tests/host_kernel/).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// A window is a run [win_off[w], win_off[w + 1]) of the SELECTED rows.  Per window and listed column, four int32 counts:
//   c0, c1, c2 = #rows with canonical code 0 / 1 / 2,  ninfo = #rows whose call is not missing (an int8 panel's code 3 included)
// and per listed pair (a, b) of columns and window:
//   n        = #rows where both calls are 0, 1 or 2        eq       = #rows among those where the two codes are equal
//   hom_same = #rows where both are homozygous and equal   hom_diff = #rows where both are homozygous and different
//
// Two kernels, run once per SLAB of selected rows (win_slab_steps below cuts the row axis):
//   k_win_planes  the scheme of k_kin_planes with a fourth plane: panel rows -> accession-major bit-planes [4][cols_pad][W] of
//       64-bit words, one bit per row: P0 = (v == 0), P1 = (v == 1), P2 = (v == 2), I = (v not missing).  A block takes 64 rows x
//       64 accessions through LDS, then with lane = row four wave64 ballots per accession ARE the four words.  Rows past the
//       slab's end and accessions past ncols give zero bits; EVERY word of [4][cols_pad][W] is written by every launch.
//   k_win_count   a work item per cell of the launch: (window of the slab, column) and (pair, window of the slab).  A group of
//       2^lg lanes takes an item and strides the words of the window's bit range in the item's plane rows (contiguous words:
//       coalesced), the first and the last word masked to the range -- a window may start and end inside one word.  Popcounts,
//       a shuffle reduction within the group, and the group's first lane stores the cell as 16 bytes.  Every cell of the launch is
//       written exactly once by its owner: no atomics, no memset.  A window spanning slabs is summed by the host.
constexpr int WN_THREADS = 256;
constexpr int WN_STEP_WORDS = 16;           // 64-bit words (= 1024 rows) per plane step; W is a multiple of it, a slab is whole steps
constexpr int64_t WN_STEP_ROWS = (int64_t)WN_STEP_WORDS * 64;
constexpr int WN_PL_ROWS = 64;              // k_win_planes: rows x accessions of a tile
constexpr int WN_PL_COLS = 64;
constexpr int WN_PL_LD = WN_PL_COLS + 4;    // bytes per LDS row of the tile (17 dwords: the 64 rows a wave reads start in different banks)
static_assert(WN_PL_ROWS == WAVE && WN_PL_COLS % (WN_THREADS / WAVE) == 0, "a ballot is a word; whole accessions per wave");
#ifndef SNPM_WIN_MAX_ACCESSIONS
#define SNPM_WIN_MAX_ACCESSIONS 4194240     // 65535 (grid.y of k_win_planes) tiles of 64 columns (include/snpmatch_hip.h carries the same figure)
#endif
static_assert(SNPM_WIN_MAX_ACCESSIONS == 65535 * WN_PL_COLS, "grid.y of k_win_planes");

__host__ __device__ __forceinline__ int64_t win_step_bytes(int64_t cols_pad) { return 4 * cols_pad * WN_STEP_WORDS * 8; }

// The host's slab plan.  The slab that starts at selected row s0 (a multiple of WN_STEP_ROWS, below n_rows): its plane steps, as
// many as the rows need and as the planes plus the cells of the slab's windows (cell_bytes per window: 16 per column and pair
// asked for) fit ws_bytes -- at least one step whatever the budget.  The slab's windows are the contiguous range [w_lo, w_end):
// from the first window that ends behind s0 to the last that starts before the slab's end, so an empty window at a slab edge
// belongs to no slab (its cells stay zero) and a window across an edge to both.  On entry w_lo is 0 or the previous slab's value.
inline int64_t win_slab_steps(size_t ws_bytes, int64_t cols_pad, int64_t cell_bytes, const int64_t *win_off, int64_t n_win, int64_t n_rows,
                              int64_t s0, int64_t &w_lo, int64_t &w_end)
{
    while (w_lo < n_win - 1 && win_off[w_lo + 1] <= s0) ++w_lo;
    const int64_t need = (n_rows - s0 + WN_STEP_ROWS - 1) / WN_STEP_ROWS, step_bytes = win_step_bytes(cols_pad);
    const double budget = (double)ws_bytes;                          // (compared in fp64: no product can overflow)
    int64_t steps = 0;
    w_end = w_lo;
    for (;;) {
        const int64_t s1 = s0 + (steps + 1) * WN_STEP_ROWS < n_rows ? s0 + (steps + 1) * WN_STEP_ROWS : n_rows;
        int64_t e = w_end;
        while (e < n_win && win_off[e] < s1) ++e;
        if (steps >= 1 && (double)(steps + 1) * (double)step_bytes + (double)(e - w_lo) * (double)cell_bytes > budget) break;
        ++steps;
        w_end = e;
        if (steps >= need) break;
    }
    return steps;
}

// lanes per work item of k_win_count, as log2: the power of two at or above the mean words of a window of the slab, 1 .. 64
inline int win_group_lg(int64_t n_valid, int64_t n_w)
{
    const int64_t words = (n_valid + 63) / 64, per = (words + n_w - 1) / (n_w > 0 ? n_w : 1);
    int lg = 0;
    while (lg < 6 && ((int64_t)1 << lg) < per) ++lg;
    return lg;
}

// grid (W, cols_pad / WN_PL_COLS).  Row k of the slab (0 <= k < n_valid) is panel row row_idx[first + k], or first + k when row_idx
// is null; column a of the call (0 <= a < ncols) is panel column cols[a], or a when cols is null.
__global__ void __launch_bounds__(WN_THREADS)
k_win_planes(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, const int64_t *__restrict__ row_idx, int64_t first, int64_t n_valid,
             const int32_t *__restrict__ cols, int64_t ncols, unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_c[WN_PL_ROWS * WN_PL_LD];       // [row][accession]
    const int64_t word = blockIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * WN_PL_COLS;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t r0 = word * WN_PL_ROWS;
    const int64_t plane = cols_pad * W;
    if (r0 >= n_valid) {                    // (block-uniform) a word of padding rows only
        if (threadIdx.x < WN_PL_COLS) {
            const int64_t at = (c0 + (int64_t)threadIdx.x) * W + word;
            planes[at] = 0ull;
            planes[plane + at] = 0ull;
            planes[2 * plane + at] = 0ull;
            planes[3 * plane + at] = 0ull;
        }
        return;
    }
    // read: a wave takes the 64 accessions of one row, the block four rows per pass
    const bool have = c0 + lane < ncols;
    const int64_t col = have ? (cols ? (int64_t)cols[c0 + lane] : c0 + lane) : 0;
#pragma unroll 4
    for (int r = wave; r < WN_PL_ROWS; r += WN_THREADS / WAVE) {
        uint32_t v = 0xFFu;
        if (have && r0 + r < n_valid) {
            const int64_t prow = row_idx ? row_idx[first + r0 + r] : first + r0 + r;
            v = kin_code(db, pitch, desc, prow, col);
        }
        s_c[r * WN_PL_LD + lane] = (uint8_t)v;
    }
    __syncthreads();
    // lane = row: a wave takes 16 accessions; lane k keeps the four words of the wave's accession k
    constexpr int per_wave = WN_PL_COLS / (WN_THREADS / WAVE);
    unsigned long long k0 = 0ull, k1 = 0ull, k2 = 0ull, ki = 0ull;
#pragma unroll 4
    for (int k = 0; k < per_wave; ++k) {
        const uint32_t v = s_c[lane * WN_PL_LD + wave * per_wave + k];
        const unsigned long long b0 = __ballot(v == 0u), b1 = __ballot(v == 1u), b2 = __ballot(v == 2u), bi = __ballot(v != 0xFFu);
        if (lane == k) { k0 = b0; k1 = b1; k2 = b2; ki = bi; }
    }
    if (lane < per_wave) {
        const int64_t at = (c0 + wave * per_wave + lane) * W + word;
        planes[at] = k0;
        planes[plane + at] = k1;
        planes[2 * plane + at] = k2;
        planes[3 * plane + at] = ki;
    }
}

__device__ __forceinline__ int win_popc(unsigned long long v) { return __popc((uint32_t)v) + __popc((uint32_t)(v >> 32)); }

// grid (blocks), any number: the blocks stride the items.  The slab holds selected rows [s0, s0 + n_valid) as bits 0 .. n_valid - 1
// of its plane rows; its windows are w_lo .. w_lo + n_w - 1 of win_off (the whole table, n_win + 1 entries).  Items 0 .. n_w * n_acc_cols
// - 1 are (window wi, column c) = (item / n_acc_cols, item % n_acc_cols) and write cells[item]; the n_pairs * n_w items behind them are
// (pair i, window wi) = (rest / n_w, rest % n_w) and write cells[item] as well: the workspace is [n_w][n_acc_cols][4] followed by
// [n_pairs][n_w][4].  n_acc_cols is ncols or 0 (columns not asked for), n_pairs may be 0.  pair_a / pair_b index the call's columns.
__global__ void __launch_bounds__(WN_THREADS)
k_win_count(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, int64_t s0, int64_t n_valid,
            const int64_t *__restrict__ win_off, int64_t w_lo, int64_t n_w, int64_t n_acc_cols, const int32_t *__restrict__ pair_a,
            const int32_t *__restrict__ pair_b, int64_t n_pairs, int lg, int32_t *__restrict__ cells)
{
    const int group = 1 << lg, per_block = WN_THREADS >> lg;
    const int gl = threadIdx.x & (group - 1);
    const int64_t acc_items = n_w * n_acc_cols, items = acc_items + n_pairs * n_w, plane = cols_pad * W;
    // (block-uniform trip count: every lane of a wave takes part in every shuffle)
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < items; base += (int64_t)gridDim.x * per_block) {
        const int64_t item = base + (threadIdx.x >> lg);
        const bool live = item < items;
        const bool is_pair = item >= acc_items;
        int64_t wi = 0, ra = 0, rb = 0;                              // window of the slab; plane rows of the column(s)
        if (live) {
            if (is_pair) {
                const int64_t rest = item - acc_items, i = rest / n_w;
                wi = rest - i * n_w;
                ra = pair_a[i];
                rb = pair_b[i];
            } else {
                wi = item / n_acc_cols;
                ra = rb = item - wi * n_acc_cols;
            }
        }
        int q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        if (live) {
            int64_t b0 = win_off[w_lo + wi] - s0, b1 = win_off[w_lo + wi + 1] - s0;      // the window's bit range in this slab
            if (b0 < 0) b0 = 0;
            if (b1 > n_valid) b1 = n_valid;
            if (b1 > b0) {
                const int64_t wf = b0 >> 6, wl = (b1 - 1) >> 6;
                const unsigned long long m_first = ~0ull << (int)(b0 & 63), m_last = ~0ull >> (63 - (int)((b1 - 1) & 63));
                const unsigned long long *pa = planes + ra * W, *pb = planes + rb * W;
                for (int64_t k = wf + gl; k <= wl; k += group) {
                    unsigned long long m = ~0ull;
                    if (k == wf) m &= m_first;
                    if (k == wl) m &= m_last;
                    const unsigned long long a0 = pa[k] & m, a1 = pa[plane + k] & m, a2 = pa[2 * plane + k] & m;
                    if (is_pair) {
                        const unsigned long long e0 = a0 & pb[k], e1 = a1 & pb[plane + k], e2 = a2 & pb[2 * plane + k];
                        const unsigned long long mb = pb[k] | pb[plane + k] | pb[2 * plane + k];
                        const int hs = win_popc(e0) + win_popc(e1);
                        q0 += win_popc((a0 | a1 | a2) & mb);
                        q1 += hs + win_popc(e2);
                        q2 += hs;
                        q3 += win_popc(a0 & pb[plane + k]) + win_popc(a1 & pb[k]);
                    } else {
                        q0 += win_popc(a0);
                        q1 += win_popc(a1);
                        q2 += win_popc(a2);
                        q3 += win_popc(pa[3 * plane + k] & m);
                    }
                }
            }
        }
        for (int s = group >> 1; s > 0; s >>= 1) {
            q0 += (int)__shfl_xor((uint32_t)q0, s);
            q1 += (int)__shfl_xor((uint32_t)q1, s);
            q2 += (int)__shfl_xor((uint32_t)q2, s);
            q3 += (int)__shfl_xor((uint32_t)q3, s);
        }
        if (live && gl == 0) {
            int4 cell;
            cell.x = q0; cell.y = q1; cell.z = q2; cell.w = q3;
            *(int4 *)(cells + 4 * item) = cell;
        }
    }
}

}  // namespace snpm
