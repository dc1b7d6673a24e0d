// snpm_k_mix.hpp -- mixture: read-count-weighted 2 x 2 tables of EVERY ordered pair of accession columns against one sample's allele depths (FORMAT AD) over panel rows: what the likelihood of "a pool of accession a with a fraction alpha of accession b" needs (the package's own: no counterpart in the reference).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp only (its planes
// come from k_win_planes of snpm_k_win.hpp, which needs kin_code of snpm_k_kin.hpp), so that tests/mix_host_driver.cpp can compile
// this very text for the host (tests/host_kernel/).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// With canonical DB codes (kin_code: 0 ref, 1 alt, 2 het, 3 other, missing) a row is informative for the ordered pair (a, b) where
// BOTH columns carry a homozygous call (0 or 1): a het, "other" or missing call on either side drops the row for that pair, as in
// kinship / ibd.  The sample has two read counts per row, alt and ref, each 0 .. 2^BITS - 1.  Per ordered pair, eight int32 sums:
//   T[w][ca][cb][a][b] = sum over rows where column a has call ca and column b has call cb of the sample's alt (w = 0) or ref (w = 1) reads
// and T[w][ca][cb][a][b] == T[w][cb][ca][b][a].
//
// Per SLAB of rows (the host cuts the row axis so that the planes fit a workspace budget):
//   planes  k_win_planes (snpm_k_win.hpp) AS IT STANDS: accession-major bit-planes [4][cols_pad][W] of 64-bit words, P0, P1, P2, I,
//       padding rows and columns as zero bits.  The scan reads P0 and P1 only.
//   masks   the sample's counts as bit slices, made by the host (mix_fill_masks: one pass over 2 n_rows bytes) in blocks of one LDS
//       step: [step][2 weights][BITS][MIX_STEP_WORDS] words -- bit k of slice j of weight w is bit j of the count at row k.
//   k_mix_count<BITS>  the scheme of k_f1x_count: grid (tile pair ta <= tb, chunk of MIX_CHUNK_WORDS words), MIX_TILE x MIX_TILE pairs
//       per block, a 2 x 2 register tile of pairs per lane, eight accumulators per pair.  A step stages TWO planes per side in LDS and
//       the 2 BITS mask rows, then per pair and 64-bit word
//         c00 = P0a & P0b   c01 = P0a & P1b   c10 = P1a & P0b   c11 = P1a & P1b
//         T[w][ca][cb] += sum_j popc(c[ca][cb] & M[w][j]) << j          (Horner over the slices: one shift-add per slice)
//       Partial sums go into the zeroed results with int32 atomicAdd (integer sums: any order, same result; zero partials are
//       skipped); a block off the diagonal also writes the mirrored cell with the class indices swapped.  The tile pair is the FAST
//       grid axis: the blocks in flight share a chunk.
constexpr int MIX_TILE = 32;                // accessions per tile side of k_mix_count
constexpr int MIX_THREADS = 256;
constexpr int MIX_STEP_WORDS = 16;          // 64-bit words (= 1024 rows, 128 B per plane row) staged in LDS at a time; W is a multiple of it
constexpr int MIX_CHUNK_WORDS = 128;        // words (= 8192 rows) per block of k_mix_count
constexpr int MIX_LD = MIX_STEP_WORDS * 2 + 4;  // dwords per LDS row: 144 bytes = 9 slots of 16 bytes, rows r and r + 1 start one slot (mod 16: nine) apart
constexpr int MIX_PLANES = 4;               // planes in memory (k_win_planes): P0, P1, P2, I
constexpr int MIX_LDS_PLANES = 2;           // planes in LDS: P0, P1
constexpr int MIX_PL_COLS = 64;             // accessions per tile of k_win_planes: cols_pad is a multiple of it
constexpr int MIX_MAX_BITS = 8;             // counts are bytes
static_assert(MIX_CHUNK_WORDS % MIX_STEP_WORDS == 0 && MIX_PL_COLS % MIX_TILE == 0, "whole steps per chunk, whole count tiles per plane tile");
static_assert(MIX_TILE * MIX_TILE == 4 * MIX_THREADS, "a 2 x 2 register tile of pairs per lane");
static_assert(MIX_TILE * MIX_STEP_WORDS * 8 / 16 == MIX_THREADS, "one 16-byte load per thread, plane and side of a step");
static_assert(2 * MIX_MAX_BITS * MIX_STEP_WORDS * 8 / 16 <= MIX_THREADS, "one 16-byte load per thread for the masks of a step");

// words of one step's masks at BITS slices per weight
__host__ __device__ constexpr int mix_mask_words(int bits) { return 2 * bits * MIX_STEP_WORDS; }
// the smallest of 2 / 4 / 8 slices that hold `max_count` (a byte)
__host__ __device__ constexpr int mix_bits_of(int max_count) { return max_count < 4 ? 2 : max_count < 16 ? 4 : 8; }

// The host's slab plan, as f1x_slab_steps: LDS steps (MIX_STEP_ROWS rows each) of one slab of an n_rows scan whose planes
// [4][cols_pad][W] must fit ws_bytes -- whole chunks where the budget holds one, at least one step, at most 65535 chunks (grid.y of
// k_mix_count) and no more than the rows need.
constexpr int64_t MIX_STEP_ROWS = (int64_t)MIX_STEP_WORDS * 64;
__host__ __device__ __forceinline__ int64_t mix_step_bytes(int64_t cols_pad) { return MIX_PLANES * cols_pad * MIX_STEP_WORDS * 8; }
__host__ __device__ __forceinline__ int64_t mix_slab_steps(size_t ws_bytes, int64_t cols_pad, int64_t n_rows)
{
    const int64_t steps_per_chunk = MIX_CHUNK_WORDS / MIX_STEP_WORDS, need = (n_rows + MIX_STEP_ROWS - 1) / MIX_STEP_ROWS;
    int64_t steps = (int64_t)(ws_bytes / (size_t)mix_step_bytes(cols_pad));
    if (steps < 1) steps = 1;
    if (steps >= steps_per_chunk) steps = steps / steps_per_chunk * steps_per_chunk;
    if (steps > 65535 * steps_per_chunk) steps = 65535 * steps_per_chunk;
    return steps < need ? steps : need;
}

// the bit slices of n_rows alt / ref counts, each below 2^bits: masks[(k / STEP_ROWS) * mix_mask_words(bits) + (w * bits + j) *
// STEP_WORDS + word of k in its step] holds, at bit k % 64, bit j of the count of weight w (0 alt, 1 ref) at row k; `masks` has
// ceil(n_rows / STEP_ROWS) * mix_mask_words(bits) words, all written (rows past n_rows: zero)
inline void mix_fill_masks(const uint8_t *alt, const uint8_t *ref, int64_t n_rows, int bits, unsigned long long *masks)
{
    const int64_t steps = (n_rows + MIX_STEP_ROWS - 1) / MIX_STEP_ROWS, mw = mix_mask_words(bits);
    for (int64_t i = 0; i < steps * mw; ++i) masks[i] = 0ull;
    for (int64_t k = 0; k < n_rows; ++k) {
        unsigned long long *at = masks + k / MIX_STEP_ROWS * mw + (k % MIX_STEP_ROWS) / 64;
        const unsigned long long bit = 1ull << (k & 63);
        const uint8_t cnt[2] = {alt[k], ref[k]};
        for (int w = 0; w < 2; ++w)
            for (int j = 0; j < bits; ++j)
                if ((cnt[w] >> j) & 1) at[(w * bits + j) * MIX_STEP_WORDS] |= bit;
    }
}

__device__ __forceinline__ int mix_popc(unsigned long long v) { return __popc((uint32_t)v) + __popc((uint32_t)(v >> 32)); }

// grid (tile pairs, chunks): blockIdx.x counts the pairs (ta, tb) with ta <= tb row by row.  out [2][2][2][ncols][ncols] (weight,
// call of a, call of b), zeroed before the first slab.  planes [4][cols_pad][W] of this slab, W a multiple of MIX_STEP_WORDS (the
// last chunk may hold fewer steps); masks: the blocks of this slab's steps, W / MIX_STEP_WORDS of them.
template <int BITS>
__global__ void __launch_bounds__(MIX_THREADS, 3)
k_mix_count(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, const unsigned long long *__restrict__ masks, int ncols,
            int n_tiles, int32_t *__restrict__ out)
{
    static_assert(BITS == 2 || BITS == 4 || BITS == 8, "2, 4 or 8 slices per count");
    constexpr int MASK_WORDS = 2 * BITS * MIX_STEP_WORDS;
    __shared__ __attribute__((aligned(16))) uint32_t s_a[MIX_LDS_PLANES * MIX_TILE * MIX_LD];      // [plane][accession][dword]
    __shared__ __attribute__((aligned(16))) uint32_t s_b[MIX_LDS_PLANES * MIX_TILE * MIX_LD];
    __shared__ __attribute__((aligned(16))) uint32_t s_m[2 * MASK_WORDS];                          // [weight][slice][dword]
    int ta = 0, rest = blockIdx.x;                                  // (block-uniform) row ta of the triangle holds n_tiles - ta pairs
    while (rest >= n_tiles - ta) { rest -= n_tiles - ta; ++ta; }
    const int tb = ta + rest;
    const bool diag = ta == tb;
    const uint32_t *sb = diag ? s_a : s_b;
    const int64_t w0 = (int64_t)blockIdx.y * MIX_CHUNK_WORDS;
    const int64_t left = (W - w0) / MIX_STEP_WORDS;
    const int steps = (int)(left < MIX_CHUNK_WORDS / MIX_STEP_WORDS ? left : MIX_CHUNK_WORDS / MIX_STEP_WORDS);
    // the lane's pairs: accessions {i, i + 16} of tile ta against {j, j + 16} of tile tb.  The 8-byte reads of a half wave: 16
    // values of j, rows 36 dwords apart -- 36 j mod 64 are the 16 multiples of 4, every read its own pair of banks; the two values of
    // i are two addresses nine slots apart, broadcast; the mask rows are one address for the whole wave
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    int acc[2][2][2][2][2];                                         // [x][y][weight][call of a][call of b]
#pragma unroll
    for (int k = 0; k < 32; ++k) (&acc[0][0][0][0][0])[k] = 0;
    const int64_t row_bytes = W * 8, plane_bytes = cols_pad * row_bytes;
    const uint8_t *base = (const uint8_t *)planes;
    const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;      // staging: one 16-byte slot of one accession per plane and side
    const int64_t ga = (int64_t)(ta * MIX_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const int64_t gb = (int64_t)(tb * MIX_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const uint4 *gm = (const uint4 *)(masks + w0 / MIX_STEP_WORDS * MASK_WORDS);
    for (int step = 0; step < steps; ++step) {
        const int64_t off = (int64_t)step * (MIX_STEP_WORDS * 8);
        {
            const uint4 v0 = *(const uint4 *)(base + ga + off), v1 = *(const uint4 *)(base + ga + plane_bytes + off);
            uint32_t *dst = s_a + srow * MIX_LD + 4 * sslot;
            *(uint4 *)(dst) = v0;
            *(uint4 *)(dst + MIX_TILE * MIX_LD) = v1;
        }
        if (!diag) {
            const uint4 v0 = *(const uint4 *)(base + gb + off), v1 = *(const uint4 *)(base + gb + plane_bytes + off);
            uint32_t *dst = s_b + srow * MIX_LD + 4 * sslot;
            *(uint4 *)(dst) = v0;
            *(uint4 *)(dst + MIX_TILE * MIX_LD) = v1;
        }
        if (threadIdx.x < MASK_WORDS / 2) *(uint4 *)(s_m + 4 * threadIdx.x) = gm[(int64_t)step * (MASK_WORDS / 2) + threadIdx.x];
        __syncthreads();
#pragma unroll 1
        for (int w = 0; w < MIX_STEP_WORDS; ++w) {                  // a 64-bit word (two dwords, one 8-byte LDS read each) at a time
            unsigned long long av[MIX_LDS_PLANES][2], bv[MIX_LDS_PLANES][2], mv[2][BITS];      // [plane][x or y], [weight][slice]
#pragma unroll
            for (int pl = 0; pl < MIX_LDS_PLANES; ++pl)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    av[pl][h] = *(const unsigned long long *)(s_a + (pl * MIX_TILE + i + 16 * h) * MIX_LD + 2 * w);
                    bv[pl][h] = *(const unsigned long long *)(sb + (pl * MIX_TILE + j + 16 * h) * MIX_LD + 2 * w);
                }
#pragma unroll
            for (int wt = 0; wt < 2; ++wt)
#pragma unroll
                for (int s = 0; s < BITS; ++s) mv[wt][s] = *(const unsigned long long *)(s_m + ((wt * BITS + s) * MIX_STEP_WORDS + w) * 2);
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int ca = 0; ca < 2; ++ca)
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb) {
                            const unsigned long long c = av[ca][x] & bv[cb][y];
#pragma unroll
                            for (int wt = 0; wt < 2; ++wt) {
                                int t = mix_popc(c & mv[wt][BITS - 1]);      // at most 64 * 255 per word
#pragma unroll
                                for (int s = BITS - 2; s >= 0; --s) t = (t << 1) + mix_popc(c & mv[wt][s]);
                                acc[x][y][wt][ca][cb] += t;
                            }
                        }
        }
        __syncthreads();
    }
    const int64_t cells = (int64_t)ncols * ncols;
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int a = ta * MIX_TILE + i + 16 * x;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int b = tb * MIX_TILE + j + 16 * y;
            if (a >= ncols || b >= ncols) continue;
            const int64_t ab = (int64_t)a * ncols + b, ba = (int64_t)b * ncols + a;
#pragma unroll
            for (int wt = 0; wt < 2; ++wt)
#pragma unroll
                for (int ca = 0; ca < 2; ++ca)
#pragma unroll
                    for (int cb = 0; cb < 2; ++cb) {
                        const int v = acc[x][y][wt][ca][cb];
                        if (v == 0) continue;
                        atomicAdd(out + ((wt * 2 + ca) * 2 + cb) * cells + ab, v);
                        if (!diag) atomicAdd(out + ((wt * 2 + cb) * 2 + ca) * cells + ba, v);
                    }
        }
    }
}

}  // namespace snpm
