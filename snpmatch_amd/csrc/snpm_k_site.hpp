// snpm_k_site.hpp -- site statistics: per-SNP allele counts per group of accessions over panel rows (Genotype.get_af_snps / calculate_af_snp_mat / _polarize_snps, core/snp_genotype.py:119-175, :360-376, :385-394 of the reference).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs pk_off and friends / WAVE of snpm_k_common.hpp
// only, so that tests/site_host_driver.cpp can compile this very text for the host (tests/host_kernel/).
#pragma once

#ifndef SNPM_SITE_MAX_GROUPS
#define SNPM_SITE_MAX_GROUPS 32             // (include/snpmatch_hip.h carries the same figure for callers)
#endif

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Per selected panel row r and group g of accession columns, four int32 counts, counts[g][r][4]:
//   c0 / c1 / c2 = members of g whose canonical code (kin_code of snpm_k_kin.hpp) is 0 / 1 / 2,  ninfo = members whose call is not
//   missing.  The int8 panel's "other" code 3 is informative and in none of c0..c2; the 2-bit value 3 and negative int8 values are
//   missing.  (int8 values above 3 do not occur in a panel: the upload stores canonical codes.)
// The only pass of the package that reduces over ACCESSIONS; one streaming read of the selected rows for all groups of the launch.
//
// Words.  A row is cut into WORDS of 32 columns, each one 32-bit lane value per indicator (code 0, code 1, code 2, informative), one
// bit per column.  A group is a bitmask over panel columns, member[g][ceil(n_acc / 32)] (bits at or beyond n_acc are zero: the pad
// bytes of a row are read by the wide loads and count for nothing, whatever they hold).  A count is popcount(indicator & member)
// summed over the words: per word and group 1 LDS read + 4 AND + 4 popcount-accumulate (packed panels have no code 3, so c0 is
// ninfo - c1 - c2 there: 3 + 3).  The indicators cost the same however many groups follow:
//   int8    a word is two 16-byte loads A, B.  Bit t of every byte of a load (t = 0, 1: the code; t = 7: missing) is taken with one
//           shift + AND per dword, and the four dwords are ORed one bit apart: byte i = 4k + j of the load lands at bit 8j + k, load B
//           four bits higher.  In the gfx950 code of a full-width row (16 loads per lane): 632 VALU from the first load to the
//           first group, addresses included -- 2.5 per byte -- and 96 per group for the eight words, reduction and store included --
//           0.4 per byte and group (budget: 5 per byte).
//   packed  a word is 8 bytes (half a 16-byte load): the low / high bits of the 16 fields of the first dword stay at even bit
//           positions, those of the second go to the odd ones: column c of the word is bit 2 (c & 15) + (c >> 4).  116 VALU for the
//           four loads (eight words) of a full-width row, 78 per group: per BYTE four times the int8 figures, so with many groups a
//           packed scan is bound by VALU, not by the read.
// Loads.  Every 16-byte load of (half) a row is issued before the first indicator is built: a chunk past the row's last one is read
// as that last one instead of being branched around (its columns are at or beyond n_acc, no group has a member there), a lane
// without a row reads the slab's first row and stores nothing.  int8 rows go in two halves of up to eight loads per lane, so that
// loads and indicators fit the 128 registers of four waves per SIMD (SITE_MIN_WAVES).
// The bit ORDER inside a word is that of the loads, not of the columns: a popcount does not care, and the block's prologue writes
// the membership words into LDS permuted the same way (site_member_word), arranged so that every lane reads its own dword.
// LDS holds the membership of all groups of the launch for the whole run of the block; nothing of it is fetched again per row.
//
// Narrow panels: a row goes to PART of a wave.  At the 1001-Genomes width a row is 72 (int8) / 18 (packed) 16-byte chunks; with a whole
// wave per row most lanes would idle and every (row, group) would pay a 6-step cross-lane reduction of four values.  Instead the host
// picks the smallest power of two S (1..64) of lanes per row for which a lane has at most SITE_CHUNKS_INT8 = 16 / SITE_CHUNKS_PACKED
// = 4 chunks (8 words either way): lane `sub` of a row takes chunks sub, S + sub, 2 S + sub, ... (every load instruction reads S x 16
// adjacent bytes of each of its 64 / S rows), a wave works on 64 / S rows at once, the counts accumulate in the lane over its words
// for free (the popcount instruction adds), and the reduction is log2 S steps of two values per group: c0 | c1 << 16 and c2 | ninfo
// << 16 share a lane value (a row total is at most SITE_MAX_ACCESSIONS < 65536).  1135 accessions: S = 8 for both formats, 8 rows per
// wave and 3 steps.  This was chosen over a transpose of partials through LDS (64 rows x 64 lanes x 2 dwords per group and wave is 32
// KiB per group) and over packing alone (which halves, not removes, the 6 steps).
//
// Eight words per lane and 64 lanes bound the width: SITE_MAX_ACCESSIONS = 16384 columns (the host refuses wider panels).  The
// indicators of a lane's row stay in registers (8 words x 4) while the groups are walked, so nothing is indexed dynamically.
// SNPM_SITE_MAX_GROUPS = 32 is bounded by LDS: 32 groups x 8 words x 64 lanes x 4 B = the 64 KiB of static LDS of a block (two blocks
// of 8 waves per CU).
//
// A wave owns whole rows; lane sub == 0 of a row writes the four counts of (row, group) with ONE 16-byte store.  No atomics, no
// memset: every cell [g][k][0..3], k < n_valid, g < n_groups, is written exactly once by the launch.
constexpr int SITE_THREADS = 512;
constexpr int SITE_MIN_WAVES = 4;           // waves per SIMD the register budget leaves room for: the two blocks per CU that LDS allows
constexpr int SITE_WORDS = 8;               // 32-column words per lane
constexpr int SITE_CHUNKS_INT8 = 16;        // 16-byte loads per lane and row: two per word
constexpr int SITE_CHUNKS_PACKED = 4;       //                                 half a load per word
constexpr int SITE_LDS_WORDS = SNPM_SITE_MAX_GROUPS * SITE_WORDS * WAVE;
constexpr int64_t SITE_MAX_ACCESSIONS = (int64_t)WAVE * SITE_WORDS * 32;
static_assert(SITE_LDS_WORDS * 4 <= 65536, "the membership words of a launch are static LDS");
static_assert(SITE_MAX_ACCESSIONS < 65536, "two counts share a 32-bit lane value");
static_assert(SITE_CHUNKS_INT8 == 2 * SITE_WORDS && 2 * SITE_CHUNKS_PACKED == SITE_WORDS, "words per lane");

// lanes per row as log2 (0..6) and 16-byte chunks per lane for a panel of n_acc accessions; false: the panel is too wide
__host__ __device__ __forceinline__ bool site_geometry(int64_t n_acc, bool packed, int *lg_s, int *cpl)
{
    const int64_t row_bytes = packed ? (n_acc + 3) / 4 : n_acc, chunks = (row_bytes + 15) / 16;
    const int64_t most = packed ? SITE_CHUNKS_PACKED : SITE_CHUNKS_INT8;
    int lg = 0;
    while (lg < 6 && (chunks + ((int64_t)1 << lg) - 1) >> lg > most) ++lg;
    *lg_s = lg;
    *cpl = (int)((chunks + ((int64_t)1 << lg) - 1) >> lg);
    return *cpl <= most;
}

// The host's slab plan: rows of one slab of an n_rows scan whose counts, 16 bytes per (group, row), must fit ws_bytes -- a multiple
// of 64, at least 64, and no more than n_rows.
__host__ __device__ __forceinline__ int64_t site_slab_rows(size_t ws_bytes, int64_t n_groups, int64_t n_rows)
{
    const int64_t fit = (int64_t)(ws_bytes / (size_t)(16 * n_groups)) / 64 * 64, rows = fit < 64 ? 64 : fit;
    return rows < n_rows ? rows : n_rows;
}

// the membership bits of word w of lane `sub` (of S = 1 << lg_s lanes per row) in the bit order of that lane's indicators.
// m: the group's bitmask over panel columns, nwords = ceil(n_acc / 32) words; words past it read as zero.
__host__ __device__ __forceinline__ uint32_t site_member_word(const uint32_t *__restrict__ m, int64_t nwords, bool packed, int lg_s, int w, int sub)
{
    uint32_t out = 0;
    if (packed) {                           // chunk (w >> 1) of the lane, its half (w & 1): columns 64 q + 32 half ..
        const int64_t q = ((int64_t)(w >> 1) << lg_s) + sub, wi = 2 * q + (w & 1);
        const uint32_t src = wi < nwords ? m[wi] : 0u;
        for (int c = 0; c < 32 && src; ++c)
            if ((src >> c) & 1u) out |= 1u << (2 * (c & 15) + (c >> 4));
        return out;
    }
    for (int h = 0; h < 2; ++h) {           // chunks 2 w and 2 w + 1 of the lane: columns 16 q ..
        const int64_t q = ((int64_t)(2 * w + h) << lg_s) + sub, wi = q >> 1;
        const uint32_t src = wi < nwords ? (m[wi] >> (16 * (int)(q & 1))) & 0xFFFFu : 0u;
        for (int i = 0; i < 16 && src; ++i)
            if ((src >> i) & 1u) out |= 1u << (8 * (i & 3) + (i >> 2) + 4 * h);
    }
    return out;
}

// bytes [16 q, 16 q + 16) of a panel row.  `main` points at byte 0 of the row in the main matrix, `tail` at where byte 0 WOULD lie
// in front of the row's part of the tail matrix (so that byte b >= split is tail[b]); split = the main pitch of a split panel, else
// beyond every row.  A chunk past the row's last one is read as that last one: its columns are at or beyond n_acc, where no group
// has a member, so its bits count for nothing -- no branch, and every load of a row can be in flight at once.  WIDE (the host's
// choice, site_wide_rows): one aligned 16-byte load -- the 16 bytes lie inside the row's pitch (of the main or the tail matrix), pad
// bytes included.  Else (a pitch that is no multiple of 16, a tail matrix below 16 bytes) byte by byte, the bytes past the row as zero.
template <bool WIDE>
__device__ __forceinline__ uint4 site_load16(const uint8_t *__restrict__ main, const uint8_t *__restrict__ tail, int split, int q, int row_bytes)
{
    const int last = (row_bytes - 1) & ~15, b = 16 * q < last ? 16 * q : last;
    const uint8_t *at = (b >= split ? tail : main) + b;
    if (WIDE) return *(const uint4 *)at;
    uint32_t d[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i)
        if (b + i < row_bytes) d[i >> 2] |= (uint32_t)at[i] << (8 * (i & 3));
    uint4 v;
    v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
    return v;
}

// every 16-byte chunk of every row starts at a 16-byte boundary and ends inside its row's pitch
__host__ __device__ __forceinline__ bool site_wide_rows(const void *db, int64_t pitch, int64_t desc)
{
    const int64_t tp = pk_tail_pitch(desc);
    return ((uintptr_t)db & 15) == 0 && (pitch & 15) == 0 && (tp & 15) == 0 && (pk_tail_off(desc) & 15) == 0;
}

// bit t of each of the 16 bytes of a load: byte i = 4 k + j (dword k, byte j) at bit 8 j + k
__device__ __forceinline__ uint32_t site_byte_bits(const uint4 v, int t)
{
    const uint32_t m = 0x01010101u;
    return ((v.x >> t) & m) | (((v.y >> t) & m) << 1) | (((v.z >> t) & m) << 2) | (((v.w >> t) & m) << 3);
}

// grid-stride over batches of 64 >> lg_s rows per wave.  Row k of the slab (0 <= k < n_valid) is panel row row_idx[first + k], or
// first + k when row_idx is null.  WIDE only where site_wide_rows() holds.  member [n_groups][ceil(n_acc / 32)]; counts [n_groups][n_valid][4].  lg_s / cpl: site_geometry.
template <bool PACKED, bool WIDE>
__global__ void __launch_bounds__(SITE_THREADS, SITE_MIN_WAVES)
k_site_counts(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, int64_t n_acc, const int64_t *__restrict__ row_idx, int64_t first,
              int64_t n_valid, const uint32_t *__restrict__ member, int n_groups, int lg_s, int cpl, int32_t *__restrict__ counts)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[SITE_LDS_WORDS];      // [group][word][sub]
    const int wl = PACKED ? 2 * cpl : (cpl + 1) / 2;                // words per lane (<= SITE_WORDS)
    const int64_t nwords = (n_acc + 31) / 32;
    for (int i = threadIdx.x; i < (n_groups * wl) << lg_s; i += SITE_THREADS) {
        const int sub = i & ((1 << lg_s) - 1), gw = i >> lg_s;
        s_mem[i] = site_member_word(member + (int64_t)(gw / wl) * nwords, nwords, PACKED, lg_s, gw % wl, sub);
    }
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int sub = lane & ((1 << lg_s) - 1), slot = lane >> lg_s, rpw = WAVE >> lg_s;
    const int row_bytes = (int)(PACKED ? (n_acc + 3) / 4 : n_acc);       // (at most SITE_MAX_ACCESSIONS)
    const int64_t n_batches = (n_valid + rpw - 1) / rpw;
    const int64_t tp = pk_tail_pitch(desc);
    const int split = tp ? (int)pitch : 0x7FFFFFFF;
    for (int64_t batch = (int64_t)blockIdx.x * (SITE_THREADS / WAVE) + wave; batch < n_batches; batch += (int64_t)gridDim.x * (SITE_THREADS / WAVE)) {
        const int64_t k = batch * rpw + slot;
        const bool have = k < n_valid;
        const int64_t prow = have ? (row_idx ? row_idx[first + k] : first + k) : (row_idx ? row_idx[first] : first);     // no row: read the slab's first, store nothing
        const uint8_t *row_main = (const uint8_t *)db + prow * pitch;
        const uint8_t *row_tail = (const uint8_t *)db + pk_tail_off(desc) + prow * tp - pitch;      // (not used without a tail matrix)
        // the loads of (half) a row first (the guards are wave-uniform), then its indicators: int8 rows in two halves of up to eight
        // loads, so that loads and indicators stay within the registers of SITE_MIN_WAVES waves per SIMD
        uint32_t e0[SITE_WORDS], e1[SITE_WORDS], e2[SITE_WORDS], ei[SITE_WORDS];
        constexpr int PHASES = PACKED ? 1 : 2, CH = (PACKED ? SITE_CHUNKS_PACKED : SITE_CHUNKS_INT8) / PHASES, WP = SITE_WORDS / PHASES;
#pragma unroll
        for (int ph = 0; ph < PHASES; ++ph) {
            if (ph * CH >= cpl) break;                              // (wave-uniform)
            uint4 ch[CH];
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                ch[j].x = ch[j].y = ch[j].z = ch[j].w = 0u;         // (the odd chunk of a last int8 word: columns past n_acc)
                if (ph * CH + j < cpl) ch[j] = site_load16<WIDE>(row_main, row_tail, split, ((ph * CH + j) << lg_s) + sub, row_bytes);
            }
#pragma unroll
            for (int u = 0; u < WP; ++u) {
                const int w = ph * WP + u;
                if (w >= wl) break;                                 // (wave-uniform)
                if (PACKED) {
                    const uint4 v = ch[u >> 1];
                    const uint32_t x0 = (u & 1) ? v.z : v.x, x1 = (u & 1) ? v.w : v.y;
                    const uint32_t lo = (x0 & 0x55555555u) | ((x1 & 0x55555555u) << 1);
                    const uint32_t hi = ((x0 >> 1) & 0x55555555u) | (x1 & 0xAAAAAAAAu);
                    e0[w] = 0u;                                     // (not used: c0 = ninfo - c1 - c2)
                    e1[w] = lo & ~hi;
                    e2[w] = hi & ~lo;
                    ei[w] = ~(lo & hi);
                } else {
                    const uint4 a = ch[(2 * u) % CH], b = ch[(2 * u + 1) % CH];
                    const uint32_t b0 = site_byte_bits(a, 0) | (site_byte_bits(b, 0) << 4);
                    const uint32_t b1 = site_byte_bits(a, 1) | (site_byte_bits(b, 1) << 4);
                    const uint32_t ms = site_byte_bits(a, 7) | (site_byte_bits(b, 7) << 4);
                    e0[w] = ~(b0 | b1 | ms);
                    e1[w] = b0 & ~b1 & ~ms;
                    e2[w] = b1 & ~b0 & ~ms;
                    ei[w] = ~ms;
                }
            }
        }
        for (int g = 0; g < n_groups; ++g) {
            const uint32_t *mg = s_mem + (((int64_t)g * wl) << lg_s) + sub;
            uint32_t c0 = 0u, c1 = 0u, c2 = 0u, ni = 0u;
#pragma unroll
            for (int w = 0; w < SITE_WORDS; ++w) {
                if (w >= wl) break;
                const uint32_t m = mg[w << lg_s];
                if (!PACKED) c0 += (uint32_t)__popc(e0[w] & m);
                c1 += (uint32_t)__popc(e1[w] & m);
                c2 += (uint32_t)__popc(e2[w] & m);
                ni += (uint32_t)__popc(ei[w] & m);
            }
            if (PACKED) c0 = ni - c1 - c2;
            uint32_t pa = c0 | (c1 << 16), pb = c2 | (ni << 16);    // a lane's partial is at most 256, a row total below 65536
            for (int o = (1 << lg_s) >> 1; o; o >>= 1) {            // (wave-uniform) the lanes of a row are S adjacent lanes
                pa += __shfl_xor(pa, o);
                pb += __shfl_xor(pb, o);
            }
            if (sub == 0 && have) {
                int4 out;
                out.x = (int)(pa & 0xFFFFu); out.y = (int)(pa >> 16); out.z = (int)(pb & 0xFFFFu); out.w = (int)(pb >> 16);
                *(int4 *)(counts + ((int64_t)g * n_valid + k) * 4) = out;
            }
        }
    }
}

}  // namespace snpm
