// snpm_k_ld.hpp -- panel LD: the nine pair counts and r2 of every selected panel row with each of the `band` rows after it (Genotype.calculate_ld / calculate_ld, core/snp_genotype.py:291-295, :348-358 of the reference, neither of which runs).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs snpm_k_common.hpp and, of snpm_k_site.hpp,
// the row loads and the word order (site_load16, site_byte_bits, site_wide_rows, site_member_word), which compile for the host as
// well: tests/ld_host_driver.cpp compiles this very text for the host (tests/host_kernel/).
#pragma once

#ifndef SNPM_LD_MAX_BAND
#define SNPM_LD_MAX_BAND 4096               // (include/snpmatch_hip.h carries the same figure for callers)
#endif

namespace snpm {
// ------------------------------------------------------------------------------------------------
// The selection is n_rows panel rows k = 0 .. n_rows - 1 (a list or a range) and a set of accession columns.  Per row three bit sets
// over the selected columns, from the canonical code (kin_code of snpm_k_kin.hpp): a = code 1 (alt), h = code 2 (het), m = code 0, 1
// or 2; the int8 panel's "other" code 3, negative int8 values and the 2-bit value 3 are outside m.  For every k and d = 1 .. band,
// j = k + d, nine int32 counts, counts[k][d - 1][9]:
//   n = |m_k & m_j|   Ak = |a_k & m_j|   Hk = |h_k & m_j|   Aj = |a_j & m_k|   Hj = |h_j & m_k|   AA = |a_k & a_j|   AH = |a_k & h_j|
//   HA = |h_k & a_j|   HH = |h_k & h_j|
// and r2[k][d - 1] from them (ld_r2 below): exact integers, three correctly rounded fp64 operations.  Cells with k + d >= n_rows hold
// zeros and NaN.  The only panel scan that reduces over accessions for PAIRS of rows; kinship is pairs of accessions over rows, site
// statistics single rows over accessions.
//
// Two kernels per slab of rows.
// k_ld_planes  the rows of the slab plus the `band` halo rows after it become member-masked planes[row][3][words] (a, h, m; words =
//   ceil(n_acc / 32), 12 bytes per 32 columns): a thread builds one word of one row with the indicator arithmetic k_site_counts
//   documents (int8: two 16-byte loads and site_byte_bits per word; packed: half a load) and ANDs the membership word in, so the
//   band kernel never sees a column outside the selection nor a pad byte.  The bit ORDER inside a word is that of the loads
//   (site_member_word with one lane per row); a popcount does not care as long as every row and the membership agree.  Every
//   word of every plane row of the slab is written by every launch: a stale workspace is never read.
// k_ld_band  one block per LD_T = 64 rows k and LD_D = 64 offsets d (grid.y walks the band): a LANE OWNS A PAIR.  Wave w of the
//   sixteen takes rows k = w, w + 16, w + 32, w + 48 of the tile, lane l the offset d = 64 blockIdx.y + l + 1, and a lane keeps
//   the nine counters of its four pairs in registers (36) over all words: no cross-lane reduction, no atomics, and the popcount
//   instruction accumulates.  Per pair and word 9 AND + 9 popcount-add; 1135 accessions are 36 words, 648 VALU per pair.
//   The 64 rows k and the 127 rows j the tile can pair them with are staged in LDS one column chunk of LD_CW = 24 words at a time
//   (coalesced loads of whole plane rows; a row past the slab's planes is staged as zeros, which is what makes the cells with
//   k + d >= n_rows zero without a branch), so that a 16 384-column row needs no more LDS than a narrow one: 64 x 72 + 127 x 73
//   dwords = 54.2 KiB of static LDS (at the 101 VGPRs of the gfx950 code one block of sixteen waves per CU).  Row k's words are
//   read by all lanes of a wave at one address (a broadcast); the other row is j = k + d, a different LDS row per lane, and the
//   rows j lie LD_PJ = 73 dwords apart: odd, so the 32 lanes that share an LDS cycle of a dword read hit the 32 banks once each.  After the last chunk a lane computes r2 of its pairs and stores whole cells (nine
//   int32, one double) with plain vector stores; every cell [k][d - 1], k < n_valid, d <= band, is written exactly once.
//   Chosen over a tile of T x band pairs per block (registers per lane grow with the band, and a halo of `band` rows per tile is
//   re-staged for few rows once the band is long) -- here the geometry does not depend on the band, at the price of idle lanes in
//   the last 64 offsets of a band that is no multiple of 64 (band 50: 22 %).
// SNPM_LD_MAX_BAND = 4096 bounds what the SMALLEST slab (64 rows, whatever the budget says) takes on the device: 64 x 4096 cells of
// 44 bytes = 11 MiB of outputs and, at 16 384 columns, 64 + 4096 plane rows of 6 KiB = 25 MiB; grid.y is 64 there.
constexpr int LD_THREADS = 1024;
constexpr int LD_T = 64;                    // rows k per block
constexpr int LD_D = 64;                    // offsets d per block: one per lane
constexpr int LD_KPL = LD_T / (LD_THREADS / WAVE);     // pairs per lane
constexpr int LD_CW = 24;                   // words of a column chunk
constexpr int LD_JROWS = LD_T + LD_D - 1;   // rows j of a block: k + d, k < LD_T, 1 <= d <= LD_D (from row 1 behind the tile's first)
constexpr int LD_PJ = 3 * LD_CW + 1;        // dwords between two rows j in LDS: odd
constexpr int LD_PLANE_THREADS = 256;
constexpr int64_t LD_MAX_ACCESSIONS = 16384;
static_assert((LD_T * 3 * LD_CW + LD_JROWS * LD_PJ) * 4 <= 65536, "a tile's column chunk is static LDS");
static_assert(LD_PJ % 2 == 1 && LD_D == WAVE && LD_T % (LD_THREADS / WAVE) == 0, "a lane per offset, whole rows per wave");

// The host's slab plan: rows k of one slab of an n_rows scan.  The slab's outputs (44 bytes per cell, `band` cells per row) and its
// planes (12 bytes per word and row, for the slab's rows and the `band` halo rows behind them) must fit ws_bytes -- a multiple of
// 64, at least 64, and no more than n_rows.
__host__ __device__ __forceinline__ int64_t ld_slab_rows(size_t ws_bytes, int64_t words, int64_t band, int64_t n_rows)
{
    const int64_t per_row = band * 44 + words * 12, halo = band * words * 12;
    const int64_t fit = (int64_t)ws_bytes > halo ? ((int64_t)ws_bytes - halo) / per_row / 64 * 64 : 0, rows = fit < 64 ? 64 : fit;
    return rows < n_rows ? rows : n_rows;
}

// r2 of one cell from its nine counts c = {n, Ak, Hk, Aj, Hj, AA, AH, HA, HH}: Pearson's r squared of the two rows' genotype values
// (v_alt for code 1, v_het for code 2, 0 for code 0) over the columns informative in both.  num, dx, dy are exact in int64 (below
// 2^33 at 16 384 columns and values up to 3), their conversions exact, so the result is three correctly rounded operations whatever
// the machine (the library is built with -ffp-contract=off; nothing here can contract anyway).  NaN: fewer than min_n common
// columns, or a row that is constant among them.
__host__ __device__ __forceinline__ double ld_r2(const int32_t *c, int v_alt, int v_het, int min_n)
{
    const int64_t n = c[0], va = v_alt, vh = v_het;
    const int64_t sx = va * c[1] + vh * c[2], sxx = va * va * c[1] + vh * vh * c[2];
    const int64_t sy = va * c[3] + vh * c[4], syy = va * va * c[3] + vh * vh * c[4];
    const int64_t sxy = va * va * c[5] + va * vh * ((int64_t)c[6] + c[7]) + vh * vh * c[8];
    const int64_t num = n * sxy - sx * sy, dx = n * sxx - sx * sx, dy = n * syy - sy * sy;
    if (n < min_n || dx == 0 || dy == 0) return __builtin_nan("");
    return ((double)num * (double)num) / ((double)dx * (double)dy);
}

// Plane row r of the slab (0 <= r < n_plane) is panel row row_idx[first + r], or first + r when row_idx is null.  member[words]:
// the selected columns in the word order of the loads (site_member_word(.., lg_s = 0, w, sub = 0)), zero at and beyond n_acc.
// WIDE only where site_wide_rows() holds.  planes [n_plane][3][words].
template <bool PACKED, bool WIDE>
__global__ void __launch_bounds__(LD_PLANE_THREADS)
k_ld_planes(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, int64_t n_acc, const int64_t *__restrict__ row_idx, int64_t first,
            int64_t n_plane, const uint32_t *__restrict__ member, int words, uint32_t *__restrict__ planes)
{
    const int row_bytes = (int)(PACKED ? (n_acc + 3) / 4 : n_acc);       // (at most LD_MAX_ACCESSIONS)
    const int64_t tp = pk_tail_pitch(desc), total = n_plane * words;
    const int split = tp ? (int)pitch : 0x7FFFFFFF;
    for (int64_t i = (int64_t)blockIdx.x * LD_PLANE_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * LD_PLANE_THREADS) {
        const int64_t r = i / words;
        const int w = (int)(i - r * words);
        const int64_t prow = row_idx ? row_idx[first + r] : first + r;
        const uint8_t *row_main = (const uint8_t *)db + prow * pitch;
        const uint8_t *row_tail = (const uint8_t *)db + pk_tail_off(desc) + prow * tp - pitch;      // (not used without a tail matrix)
        uint32_t a, h, m;
        if (PACKED) {
            const uint4 v = site_load16<WIDE>(row_main, row_tail, split, w >> 1, row_bytes);
            const uint32_t x0 = (w & 1) ? v.z : v.x, x1 = (w & 1) ? v.w : v.y;
            const uint32_t lo = (x0 & 0x55555555u) | ((x1 & 0x55555555u) << 1);
            const uint32_t hi = ((x0 >> 1) & 0x55555555u) | (x1 & 0xAAAAAAAAu);
            a = lo & ~hi; h = hi & ~lo; m = ~(lo & hi);
        } else {
            const uint4 va = site_load16<WIDE>(row_main, row_tail, split, 2 * w, row_bytes);
            const uint4 vb = site_load16<WIDE>(row_main, row_tail, split, 2 * w + 1, row_bytes);
            const uint32_t b0 = site_byte_bits(va, 0) | (site_byte_bits(vb, 0) << 4);
            const uint32_t b1 = site_byte_bits(va, 1) | (site_byte_bits(vb, 1) << 4);
            const uint32_t ms = site_byte_bits(va, 7) | (site_byte_bits(vb, 7) << 4);
            a = b0 & ~b1 & ~ms; h = b1 & ~b0 & ~ms; m = ~(b0 & b1) & ~ms;
        }
        const uint32_t mem = member[w];
        uint32_t *out = planes + r * 3 * words + w;
        out[0] = a & mem;
        out[words] = h & mem;
        out[2 * (int64_t)words] = m & mem;
    }
}

// grid (ceil(n_valid / LD_T), ceil(band / LD_D)).  planes [n_plane][3][words]: the slab's n_valid rows and its halo, n_plane <=
// n_valid + band (fewer where the selection ends: those cells come out zero / NaN).  counts [n_valid][band][9] and r2
// [n_valid][band]; either may be null.
__global__ void __launch_bounds__(LD_THREADS)
k_ld_band(const uint32_t *__restrict__ planes, int words, int64_t n_plane, int64_t n_valid, int64_t band, int v_alt, int v_het, int min_n,
          int32_t *__restrict__ counts, double *__restrict__ r2)
{
    __shared__ uint32_t s_k[LD_T * 3 * LD_CW];          // [row k][plane][word of the chunk]
    __shared__ uint32_t s_j[LD_JROWS * LD_PJ];          // [row j][plane][word of the chunk], rows LD_PJ dwords apart
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * LD_T, d0 = (int64_t)blockIdx.y * LD_D, j0 = t0 + d0 + 1;
    uint32_t c[LD_KPL][9];
#pragma unroll
    for (int i = 0; i < LD_KPL; ++i)
#pragma unroll
        for (int q = 0; q < 9; ++q) c[i][q] = 0u;
    for (int w0 = 0; w0 < words; w0 += LD_CW) {
        const int cw = words - w0 < LD_CW ? words - w0 : LD_CW, per_row = 3 * cw;
        for (int i = threadIdx.x; i < (LD_T + LD_JROWS) * per_row; i += LD_THREADS) {
            const int row = i / per_row, rem = i - row * per_row, p = rem / cw, w = rem - p * cw;
            const int64_t g = row < LD_T ? t0 + row : j0 + (row - LD_T);
            const uint32_t v = g < n_plane ? planes[(g * 3 + p) * words + w0 + w] : 0u;
            if (row < LD_T) s_k[row * (3 * LD_CW) + p * LD_CW + w] = v;
            else s_j[(row - LD_T) * LD_PJ + p * LD_CW + w] = v;
        }
        __syncthreads();
        for (int w = 0; w < cw; ++w) {
#pragma unroll
            for (int i = 0; i < LD_KPL; ++i) {
                const int kl = wave + i * (LD_THREADS / WAVE);
                const uint32_t *rk = s_k + kl * (3 * LD_CW) + w, *rj = s_j + (kl + lane) * LD_PJ + w;
                const uint32_t ak = rk[0], hk = rk[LD_CW], mk = rk[2 * LD_CW], aj = rj[0], hj = rj[LD_CW], mj = rj[2 * LD_CW];
                c[i][0] += (uint32_t)__popc(mk & mj);
                c[i][1] += (uint32_t)__popc(ak & mj);
                c[i][2] += (uint32_t)__popc(hk & mj);
                c[i][3] += (uint32_t)__popc(aj & mk);
                c[i][4] += (uint32_t)__popc(hj & mk);
                c[i][5] += (uint32_t)__popc(ak & aj);
                c[i][6] += (uint32_t)__popc(ak & hj);
                c[i][7] += (uint32_t)__popc(hk & aj);
                c[i][8] += (uint32_t)__popc(hk & hj);
            }
        }
        __syncthreads();                                // the next chunk overwrites what the slowest wave may still read
    }
    const int64_t d = d0 + lane + 1;
#pragma unroll
    for (int i = 0; i < LD_KPL; ++i) {
        const int64_t k = t0 + wave + i * (LD_THREADS / WAVE);
        if (k >= n_valid || d > band) continue;
        const int64_t cell = k * band + (d - 1);
        int32_t v[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) v[q] = (int32_t)c[i][q];
        if (counts) {
#pragma unroll
            for (int q = 0; q < 9; ++q) counts[cell * 9 + q] = v[q];
        }
        if (r2) r2[cell] = ld_r2(v, v_alt, v_het, min_n);
    }
}

}  // namespace snpm
