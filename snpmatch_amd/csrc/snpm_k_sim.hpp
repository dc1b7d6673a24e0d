// snpm_k_sim.hpp -- power: a sample SIMULATED from every accession column (its calls at the selected rows, with call errors injected by a counter-based hash) scored against every accession column, per group of selected rows (the all-accessions form of simulateSNPs + inbred, core/simulate.py:26-53 and core/snpmatch.py:74-117 of the reference, which take one accession and one marker count at a time).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp, k_win_planes of
// snpm_k_win.hpp (its planes) and the constants and f1x_popc of snpm_k_f1x.hpp only, so that tests/sim_host_driver.cpp can compile
// this very text for the host (tests/host_kernel/).
#pragma once
#include <cstdint>

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Columns a, b are POSITIONS in the column list, k is the POSITION of a row in the selected rows, codes are canonical (kin_code: 0 ref,
// 1 alt, 2 het, 3 other, missing).  The sample simulated from a has a call at k when a's code there is 0, 1 or 2; its class is that
// code unless (h >> 32) < err_thr, h = sim_hash(seed, a, k): then it is ((h & 0xFFFFFFFF) * 3) >> 32, which may be the code itself.
// err_thr is 0 .. 2^32: the error rate times 2^32.  Groups are runs [grp_off[g], grp_off[g + 1]) of the selected rows.  Per group and
// ORDERED pair, two int32 counts:
//   ninfo[g][a][b] = #rows of g where sample a has a call and b's code is not missing (code 3 counts)
//   score[g][a][b] = #rows of g where b's code is sample a's class
// With the one-hot weights of the sample these are the reference's NumInfoSites / ScoreList.  The matrices are not symmetric.
//
// Per SLAB of rows (sim_slab_steps: SEVEN planes of a slab fit the workspace budget):
//   planes  k_win_planes AS IT STANDS: [4][cols_pad][W] words, P0, P1, P2, I; padding rows and columns are zero bits.
//   k_sim_noise  the sample planes Q0, Q1, Q2 [3][cols_pad][W] from P0, P1, P2: a thread per (column, word) hashes the bits set in
//       P0 | P1 | P2 only and moves a bit to another plane where the hash says so.  Every word of Q is written by every launch
//       (padding: zero, as P is there).  Not launched when err_thr == 0: side A of the count then reads P itself.
//   k_sim_count  the tiling of k_f1x_count -- F1X_TILE x F1X_TILE pairs per block of 256 threads, a 2 x 2 register tile per lane, steps
//       of F1X_STEP_WORDS words, chunks of F1X_CHUNK_WORDS words, F1X_LD dwords per LDS row -- over the FULL square of tile pairs
//       (a diagonal block stages both sides as well: Q is not P).  Side A stages Q0, Q1, Q2 and E = Q0 | Q1 | Q2 (made while staging),
//       side B P0, P1, P2, I: 4 + 4 planes, 36 KiB of LDS.  Per pair and word
//         eq = (Q0a & P0b) | (Q1a & P1b) | (Q2a & P2b)     score += popc(eq)     ninfo += popc(Ea & Ib)
//       The block walks its words with a block-uniform group cursor into grp_off.  A step without a boundary inside takes the
//       unmasked loop; else a word is cut by bit masks into the parts before and behind each boundary (several may fall into one
//       word).  When the cursor leaves a group the lanes add their eight counters into out[g] with int32 atomicAdd (integer sums:
//       any order, same result; zero partials are skipped) and clear them; empty groups flush nothing.  No mirrored writes.
//   gfx950: k_sim_count takes 105 VGPRs under __launch_bounds__(256, 4) (four blocks per CU is what the LDS allows: 128 registers a
//   lane), k_sim_noise 22 under __launch_bounds__(256); no scratch, no spills.  No inline assembly, no floating point.
constexpr int SIM_THREADS = F1X_THREADS;
constexpr int SIM_MIN_BLOCKS = 4;           // blocks per CU the register budget is set for: the four that 36 KiB of LDS each allow
constexpr int SIM_PLANES = 7;               // planes of a slab in memory: P0, P1, P2, I (k_win_planes) and Q0, Q1, Q2 (k_sim_noise)
constexpr int SIM_LDS_PLANES = 4;           // planes per side in LDS
constexpr int SIM_MAX_GROUPS = 64;
#ifndef SNPM_SIM_MAX_ACCESSIONS
#define SNPM_SIM_MAX_ACCESSIONS 11552       // 361 tiles of 32: grid.x of k_sim_count is 361^2 (include/snpmatch_hip.h carries the same figure)
#endif
static_assert((SNPM_SIM_MAX_ACCESSIONS + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS / (SIM_THREADS / WAVE) <= 65535, "grid.y of k_sim_noise: a padded column per wave");

// The counter-based hash of (seed, column position a, selected-row position k): one round of the splitmix64 finaliser over the
// column's key seed + 0x9E3779B97F4A7C15 (a + 1), the row position xor-ed in, a second round.  All arithmetic modulo 2^64.
// tests/power_twin.py restates it with numpy.
__host__ __device__ __forceinline__ uint64_t sim_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t sim_col_key(uint64_t seed, uint64_t a) { return sim_mix(seed + 0x9E3779B97F4A7C15ull * (a + 1)); }
__host__ __device__ __forceinline__ uint64_t sim_hash(uint64_t seed, uint64_t a, uint64_t k) { return sim_mix(sim_col_key(seed, a) ^ k); }

// The host's slab plan, as f1x_slab_steps with seven planes: LDS steps of one slab of an n_rows scan.
__host__ __device__ __forceinline__ int64_t sim_step_bytes(int64_t cols_pad) { return SIM_PLANES * cols_pad * F1X_STEP_WORDS * 8; }
__host__ __device__ __forceinline__ int64_t sim_slab_steps(size_t ws_bytes, int64_t cols_pad, int64_t n_rows)
{
    const int64_t steps_per_chunk = F1X_CHUNK_WORDS / F1X_STEP_WORDS, need = (n_rows + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS;
    int64_t steps = (int64_t)(ws_bytes / (size_t)sim_step_bytes(cols_pad));
    if (steps < 1) steps = 1;
    if (steps >= steps_per_chunk) steps = steps / steps_per_chunk * steps_per_chunk;
    if (steps > 65535 * steps_per_chunk) steps = 65535 * steps_per_chunk;
    return steps < need ? steps : need;
}

// grid (ceil(W / 64), cols_pad / 4): a wave takes 64 words of one column.  planes [4][cols_pad][W] of this slab (P0, P1, P2 are
// read), q [3][cols_pad][W]; bit 0 of word 0 is selected row s0.  err_thr 1 .. 2^32.
__global__ void __launch_bounds__(SIM_THREADS)
k_sim_noise(const unsigned long long *__restrict__ planes, unsigned long long *__restrict__ q, int64_t cols_pad, int64_t W, int64_t s0,
            unsigned long long err_thr, unsigned long long seed)
{
    const int64_t word = (int64_t)blockIdx.x * WAVE + (threadIdx.x & (WAVE - 1));
    const int64_t col = (int64_t)blockIdx.y * (SIM_THREADS / WAVE) + (threadIdx.x >> 6);
    if (word >= W || col >= cols_pad) return;
    const int64_t plane = cols_pad * W, at = col * W + word;
    unsigned long long q0 = planes[at], q1 = planes[plane + at], q2 = planes[2 * plane + at];
    const uint64_t key = sim_col_key(seed, (uint64_t)col), k0 = (uint64_t)(s0 + word * 64);
    for (unsigned long long m = q0 | q1 | q2; m; m &= m - 1) {       // the calls of this word, lowest first
        const int bit = __builtin_ctzll(m);
        const uint64_t h = sim_mix(key ^ (k0 + (uint64_t)bit));
        if ((h >> 32) >= err_thr) continue;
        const uint32_t c = (uint32_t)(((h & 0xFFFFFFFFull) * 3ull) >> 32);
        const unsigned long long b = 1ull << bit;
        q0 = c == 0u ? q0 | b : q0 & ~b;
        q1 = c == 1u ? q1 | b : q1 & ~b;
        q2 = c == 2u ? q2 | b : q2 & ~b;
    }
    q[at] = q0;
    q[plane + at] = q1;
    q[2 * plane + at] = q2;
}

// one 64-bit word of the staged step: the lane's 2 x 2 pairs, side A under `mask` when MASKED
template <bool MASKED>
__device__ __forceinline__ void sim_word(const uint32_t *s_a, const uint32_t *s_b, int i, int j, int w, unsigned long long mask, int (&sc)[2][2], int (&ni)[2][2])
{
    unsigned long long av[SIM_LDS_PLANES][2], bv[SIM_LDS_PLANES][2];      // [plane][x or y]
#pragma unroll
    for (int pl = 0; pl < SIM_LDS_PLANES; ++pl)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            av[pl][h] = *(const unsigned long long *)(s_a + (pl * F1X_TILE + i + 16 * h) * F1X_LD + 2 * w);
            bv[pl][h] = *(const unsigned long long *)(s_b + (pl * F1X_TILE + j + 16 * h) * F1X_LD + 2 * w);
            if (MASKED) av[pl][h] &= mask;
        }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const unsigned long long eq = (av[0][x] & bv[0][y]) | (av[1][x] & bv[1][y]) | (av[2][x] & bv[2][y]);
            sc[x][y] += f1x_popc(eq);
            ni[x][y] += f1x_popc(av[3][x] & bv[3][y]);
        }
}

// the lane's counters into the cells of group g, then cleared; zero partials are skipped (score <= ninfo)
__device__ __forceinline__ void sim_flush(int32_t *out_score, int32_t *out_ninfo, int64_t g, int ncols, int a0, int b0, int (&sc)[2][2], int (&ni)[2][2])
{
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int a = a0 + 16 * x, b = b0 + 16 * y;
            if (ni[x][y] != 0 && a < ncols && b < ncols) {
                const int64_t at = (g * ncols + a) * (int64_t)ncols + b;
                atomicAdd(out_ninfo + at, ni[x][y]);
                if (sc[x][y]) atomicAdd(out_score + at, sc[x][y]);
            }
            sc[x][y] = ni[x][y] = 0;
        }
}

// grid (n_tiles^2, chunks): blockIdx.x = ta * n_tiles + tb, side A (the samples) tile ta, side B (the DB) tile tb.  out_* [n_grp][ncols]
// [ncols], zeroed before the first slab.  pplanes [4][cols_pad][W] of this slab; qplanes the three sample planes with the same
// strides (pplanes itself when no error is injected); W a multiple of F1X_STEP_WORDS; bit 0 of word 0 is selected row s0.
// grp_off [n_grp + 1]: starts at 0, never decreases; rows at or behind grp_off[n_grp] are padding (zero bits).
__global__ void __launch_bounds__(SIM_THREADS, SIM_MIN_BLOCKS)
k_sim_count(const unsigned long long *__restrict__ pplanes, const unsigned long long *__restrict__ qplanes, int64_t cols_pad, int64_t W, int64_t s0,
            const int64_t *__restrict__ grp_off, int n_grp, int ncols, int n_tiles, int32_t *__restrict__ out_score, int32_t *__restrict__ out_ninfo)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_a[SIM_LDS_PLANES * F1X_TILE * F1X_LD];      // [Q0, Q1, Q2, E][accession][dword]
    __shared__ __attribute__((aligned(16))) uint32_t s_b[SIM_LDS_PLANES * F1X_TILE * F1X_LD];      // [P0, P1, P2, I][accession][dword]
    const int ta = (int)(blockIdx.x / (unsigned)n_tiles), tb = (int)(blockIdx.x % (unsigned)n_tiles);
    const int64_t w0 = (int64_t)blockIdx.y * F1X_CHUNK_WORDS;
    const int64_t left = (W - w0) / F1X_STEP_WORDS;
    const int steps = (int)(left < F1X_CHUNK_WORDS / F1X_STEP_WORDS ? left : F1X_CHUNK_WORDS / F1X_STEP_WORDS);
    // the lane's pairs and its staging slot: as in k_f1x_count
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int a0 = ta * F1X_TILE + i, b0 = tb * F1X_TILE + j;
    int sc[2][2] = {{0, 0}, {0, 0}}, ni[2][2] = {{0, 0}, {0, 0}};
    const int64_t row_bytes = W * 8, plane_bytes = cols_pad * row_bytes;
    const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;
    const uint8_t *ga = (const uint8_t *)qplanes + (int64_t)(ta * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const uint8_t *gb = (const uint8_t *)pplanes + (int64_t)(tb * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    int64_t g = 0;                                                   // (block-uniform) the group of the row the walk stands at
    for (int step = 0; step < steps; ++step) {
        const int64_t off = (int64_t)step * (F1X_STEP_WORDS * 8);
        {
            const uint4 v0 = *(const uint4 *)(ga + off), v1 = *(const uint4 *)(ga + plane_bytes + off), v2 = *(const uint4 *)(ga + 2 * plane_bytes + off);
            uint4 e;
            e.x = v0.x | v1.x | v2.x; e.y = v0.y | v1.y | v2.y; e.z = v0.z | v1.z | v2.z; e.w = v0.w | v1.w | v2.w;
            uint32_t *dst = s_a + srow * F1X_LD + 4 * sslot;
            *(uint4 *)(dst) = v0;
            *(uint4 *)(dst + F1X_TILE * F1X_LD) = v1;
            *(uint4 *)(dst + 2 * F1X_TILE * F1X_LD) = v2;
            *(uint4 *)(dst + 3 * F1X_TILE * F1X_LD) = e;
        }
        {
            uint32_t *dst = s_b + srow * F1X_LD + 4 * sslot;
#pragma unroll
            for (int pl = 0; pl < F1X_PLANES; ++pl) *(uint4 *)(dst + pl * F1X_TILE * F1X_LD) = *(const uint4 *)(gb + pl * plane_bytes + off);
        }
        __syncthreads();
        const int64_t r0 = s0 + (w0 + (int64_t)step * F1X_STEP_WORDS) * 64;      // the step's first selected row
        while (g < n_grp - 1 && grp_off[g + 1] <= r0) {              // groups that ended at or before it (empty ones among them)
            sim_flush(out_score, out_ninfo, g, ncols, a0, b0, sc, ni);
            ++g;
        }
        if (g == n_grp - 1 || grp_off[g + 1] >= r0 + F1X_STEP_ROWS) {            // no boundary inside the step
#pragma unroll 2
            for (int w = 0; w < F1X_STEP_WORDS; ++w) sim_word<false>(s_a, s_b, i, j, w, ~0ull, sc, ni);
        } else {
            for (int w = 0; w < F1X_STEP_WORDS; ++w) {
                const int64_t rw = r0 + (int64_t)w * 64;
                int lo = 0;                                          // bits of this word below lo are counted
                while (lo < 64) {
                    while (g < n_grp - 1 && grp_off[g + 1] <= rw + lo) {
                        sim_flush(out_score, out_ninfo, g, ncols, a0, b0, sc, ni);
                        ++g;
                    }
                    const int64_t end = g == n_grp - 1 ? (int64_t)64 : grp_off[g + 1] - rw;
                    const int hi = end < 64 ? (int)end : 64;         // (lo < hi: the cursor's group ends behind rw + lo)
                    const unsigned long long mask = (~0ull << lo) & (hi == 64 ? ~0ull : ~(~0ull << hi));
                    sim_word<true>(s_a, s_b, i, j, w, mask, sc, ni);
                    lo = hi;
                }
            }
        }
        __syncthreads();
    }
    sim_flush(out_score, out_ninfo, g, ncols, a0, b0, sc, ni);
}

}  // namespace snpm
