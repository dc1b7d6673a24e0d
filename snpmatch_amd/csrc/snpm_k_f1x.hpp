// snpm_k_f1x.hpp -- f1search: the in-silico F1 of EVERY pair of accession columns scored against one sample's hard calls over panel rows (the exhaustive form of CrossIdentifier.match_insilico_f1s, core/csmatch.py:106-129 of the reference, which crosses the ten best single accessions only).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp only (its planes
// come from k_win_planes of snpm_k_win.hpp, which needs kin_code of snpm_k_kin.hpp), so that tests/f1x_host_driver.cpp can compile
// this very text for the host (tests/host_kernel/).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// With canonical DB codes (kin_code: 0 ref, 1 alt, 2 het, 3 other, missing) the F1 of columns a, b at a row is
//   ref  both codes 0        alt  both codes 1        het  both not missing and the codes differ
//   uninformative otherwise: a call missing, 2 with 2, 3 with 3 (the rule of snpm_query_f1_pairs, include/snpmatch_hip.h)
// and the sample has one class per row: 0 ref, 1 alt, 2 het, 0xFF none.  Per pair, two int32 counts:
//   ninfo[a, b] = #rows where the F1 is ref, alt or het        hits[a, b] = #rows where the F1's class is the sample's class
//
// Per SLAB of rows (the host cuts the row axis so that the planes fit a workspace budget):
//   planes  k_win_planes (snpm_k_win.hpp) AS IT STANDS: accession-major bit-planes [4][cols_pad][W] of 64-bit words, P0, P1, P2, I.
//       They are the planes this scan needs -- P3 = I & ~(P0 | P1 | P2) is two operations per staged word -- and that kernel writes
//       every word of the slab's planes in every launch, padding rows and columns as zero bits.
//   masks   the sample's classes as three bit masks S0, S1, S2, made by the host (f1x_fill_masks: one pass over n_rows bytes; 3 bits
//       per row travel) in blocks of one LDS step: [step][3][F1X_STEP_WORDS] words, so a step's masks are 384 contiguous bytes.
//   k_f1x_count  the scheme of k_kin_count: grid (tile pair ta <= tb, chunk of F1X_CHUNK_WORDS words), F1X_TILE x F1X_TILE pairs per
//       block, a 2 x 2 register tile of pairs per lane.  A step stages FIVE planes per side in LDS (P0, P1, P2, P3, I; P3 made
//       while staging) and the three mask rows, then per pair and dword
//         e0 = P0a & P0b   e1 = P1a & P1b   u = (P2a & P2b) | (P3a & P3b)   ni = (Ia & Ib) ^ u      (u lies inside Ia & Ib)
//         het = ni ^ e0 ^ e1                                                (e0, e1 disjoint, inside ni)
//         ninfo += popc(ni)   hits += popc((e0 & S0) | (e1 & S1) | (het & S2))                         (disjoint terms)
//       i.e. 12 logic operations (5 AND, AND-OR, 3 XOR, AND, 2 AND-OR) and 2 popcount-accumulates per pair and dword as written
//       (the gfx950 code: 8 AND, 3 XOR, OR, OR3, 2 BCNT, ADD3), walked a 64-bit word at a time -- with 16-byte reads written out two
//       iterations' planes stay live, more than the register file holds at three waves per SIMD.  Partial
//       counts go into the zeroed results with int32 atomicAdd (integer sums: any order, same result; zero partials are skipped); a
//       block off the diagonal also writes the mirrored cell.  The tile pair is the FAST grid axis: the blocks in flight share a chunk.
constexpr int F1X_TILE = 32;                // accessions per tile side of k_f1x_count
constexpr int F1X_THREADS = 256;
constexpr int F1X_STEP_WORDS = 16;          // 64-bit words (= 1024 rows, 128 B per plane row) staged in LDS at a time; W is a multiple of it
constexpr int F1X_CHUNK_WORDS = 128;        // words (= 8192 rows) per block of k_f1x_count
constexpr int F1X_LD = F1X_STEP_WORDS * 2 + 4;  // dwords per LDS row: 144 bytes = 9 slots of 16 bytes, rows r and r + 1 start one slot (mod 16: nine) apart
constexpr int F1X_PLANES = 4;               // planes in memory (k_win_planes): P0, P1, P2, I
constexpr int F1X_LDS_PLANES = 5;           // planes in LDS: P0, P1, P2, P3, I
constexpr int F1X_PL_COLS = 64;             // accessions per tile of k_win_planes: cols_pad is a multiple of it
constexpr int F1X_MASK_WORDS = 3 * F1X_STEP_WORDS;     // words of one step's masks
static_assert(F1X_CHUNK_WORDS % F1X_STEP_WORDS == 0 && F1X_PL_COLS % F1X_TILE == 0, "whole steps per chunk, whole count tiles per plane tile");
static_assert(F1X_TILE * F1X_TILE == 4 * F1X_THREADS, "a 2 x 2 register tile of pairs per lane");
static_assert(F1X_TILE * F1X_STEP_WORDS * 8 / 16 == F1X_THREADS, "one 16-byte load per thread, plane and side of a step");
static_assert(F1X_MASK_WORDS * 8 / 16 <= F1X_THREADS, "one 16-byte load per thread for the masks of a step");

// The host's slab plan, as kin_slab_steps: LDS steps (F1X_STEP_ROWS rows each) of one slab of an n_rows scan whose planes
// [4][cols_pad][W] must fit ws_bytes -- whole chunks where the budget holds one, at least one step, at most 65535 chunks (grid.y of
// k_f1x_count) and no more than the rows need.
constexpr int64_t F1X_STEP_ROWS = (int64_t)F1X_STEP_WORDS * 64;
__host__ __device__ __forceinline__ int64_t f1x_step_bytes(int64_t cols_pad) { return F1X_PLANES * cols_pad * F1X_STEP_WORDS * 8; }
__host__ __device__ __forceinline__ int64_t f1x_slab_steps(size_t ws_bytes, int64_t cols_pad, int64_t n_rows)
{
    const int64_t steps_per_chunk = F1X_CHUNK_WORDS / F1X_STEP_WORDS, need = (n_rows + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS;
    int64_t steps = (int64_t)(ws_bytes / (size_t)f1x_step_bytes(cols_pad));
    if (steps < 1) steps = 1;
    if (steps >= steps_per_chunk) steps = steps / steps_per_chunk * steps_per_chunk;
    if (steps > 65535 * steps_per_chunk) steps = 65535 * steps_per_chunk;
    return steps < need ? steps : need;
}

// the masks of n_rows classes (0 / 1 / 2, anything else: no class): masks[(k / STEP_ROWS) * MASK_WORDS + c * STEP_WORDS + word of k in
// its step] holds bit k % 64 of class c; `masks` has ceil(n_rows / STEP_ROWS) * MASK_WORDS words, all written (rows past n_rows: zero)
inline void f1x_fill_masks(const uint8_t *sample_class, int64_t n_rows, unsigned long long *masks)
{
    const int64_t steps = (n_rows + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS;
    for (int64_t i = 0; i < steps * F1X_MASK_WORDS; ++i) masks[i] = 0ull;
    for (int64_t k = 0; k < n_rows; ++k) {
        const uint8_t c = sample_class[k];
        if (c > 2) continue;
        masks[k / F1X_STEP_ROWS * F1X_MASK_WORDS + c * F1X_STEP_WORDS + (k % F1X_STEP_ROWS) / 64] |= 1ull << (k & 63);
    }
}

__device__ __forceinline__ int f1x_popc(unsigned long long v) { return __popc((uint32_t)v) + __popc((uint32_t)(v >> 32)); }

// grid (tile pairs, chunks): blockIdx.x counts the pairs (ta, tb) with ta <= tb row by row.  out_* [ncols, ncols], zeroed before the
// first slab.  planes [4][cols_pad][W] of this slab, W a multiple of F1X_STEP_WORDS (the last chunk may hold fewer steps); masks:
// the blocks of this slab's steps, W / F1X_STEP_WORDS of them.
__global__ void __launch_bounds__(F1X_THREADS, 3)
k_f1x_count(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, const unsigned long long *__restrict__ masks, int ncols,
            int n_tiles, int32_t *__restrict__ out_hits, int32_t *__restrict__ out_ninfo)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_a[F1X_LDS_PLANES * F1X_TILE * F1X_LD];      // [plane][accession][dword]
    __shared__ __attribute__((aligned(16))) uint32_t s_b[F1X_LDS_PLANES * F1X_TILE * F1X_LD];
    __shared__ __attribute__((aligned(16))) uint32_t s_m[2 * F1X_MASK_WORDS];                      // [class][dword]
    int ta = 0, rest = blockIdx.x;                                  // (block-uniform) row ta of the triangle holds n_tiles - ta pairs
    while (rest >= n_tiles - ta) { rest -= n_tiles - ta; ++ta; }
    const int tb = ta + rest;
    const bool diag = ta == tb;
    const uint32_t *sb = diag ? s_a : s_b;
    const int64_t w0 = (int64_t)blockIdx.y * F1X_CHUNK_WORDS;
    const int64_t left = (W - w0) / F1X_STEP_WORDS;
    const int steps = (int)(left < F1X_CHUNK_WORDS / F1X_STEP_WORDS ? left : F1X_CHUNK_WORDS / F1X_STEP_WORDS);
    // the lane's pairs: accessions {i, i + 16} of tile ta against {j, j + 16} of tile tb.  The 8-byte reads of a half wave: 16
    // values of j, rows 36 dwords apart -- 36 j mod 64 are the 16 multiples of 4, every read its own pair of banks; the two values of
    // i are two addresses nine slots apart, broadcast; the mask rows are one address for the whole wave)
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    int hit[2][2] = {{0, 0}, {0, 0}}, nin[2][2] = {{0, 0}, {0, 0}};
    const int64_t row_bytes = W * 8, plane_bytes = cols_pad * row_bytes;
    const uint8_t *base = (const uint8_t *)planes;
    const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;      // staging: one 16-byte slot of one accession per plane and side
    const int64_t ga = (int64_t)(ta * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const int64_t gb = (int64_t)(tb * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const uint4 *gm = (const uint4 *)(masks + w0 / F1X_STEP_WORDS * F1X_MASK_WORDS);
    for (int step = 0; step < steps; ++step) {
        const int64_t off = (int64_t)step * (F1X_STEP_WORDS * 8);
        {
            uint4 v[F1X_PLANES];
#pragma unroll
            for (int pl = 0; pl < F1X_PLANES; ++pl) v[pl] = *(const uint4 *)(base + ga + pl * plane_bytes + off);
            uint4 p3;
            p3.x = v[3].x & ~(v[0].x | v[1].x | v[2].x); p3.y = v[3].y & ~(v[0].y | v[1].y | v[2].y);
            p3.z = v[3].z & ~(v[0].z | v[1].z | v[2].z); p3.w = v[3].w & ~(v[0].w | v[1].w | v[2].w);
            uint32_t *dst = s_a + srow * F1X_LD + 4 * sslot;
            *(uint4 *)(dst) = v[0];
            *(uint4 *)(dst + F1X_TILE * F1X_LD) = v[1];
            *(uint4 *)(dst + 2 * F1X_TILE * F1X_LD) = v[2];
            *(uint4 *)(dst + 3 * F1X_TILE * F1X_LD) = p3;
            *(uint4 *)(dst + 4 * F1X_TILE * F1X_LD) = v[3];
        }
        if (!diag) {
            uint4 v[F1X_PLANES];
#pragma unroll
            for (int pl = 0; pl < F1X_PLANES; ++pl) v[pl] = *(const uint4 *)(base + gb + pl * plane_bytes + off);
            uint4 p3;
            p3.x = v[3].x & ~(v[0].x | v[1].x | v[2].x); p3.y = v[3].y & ~(v[0].y | v[1].y | v[2].y);
            p3.z = v[3].z & ~(v[0].z | v[1].z | v[2].z); p3.w = v[3].w & ~(v[0].w | v[1].w | v[2].w);
            uint32_t *dst = s_b + srow * F1X_LD + 4 * sslot;
            *(uint4 *)(dst) = v[0];
            *(uint4 *)(dst + F1X_TILE * F1X_LD) = v[1];
            *(uint4 *)(dst + 2 * F1X_TILE * F1X_LD) = v[2];
            *(uint4 *)(dst + 3 * F1X_TILE * F1X_LD) = p3;
            *(uint4 *)(dst + 4 * F1X_TILE * F1X_LD) = v[3];
        }
        if (threadIdx.x < F1X_MASK_WORDS / 2) *(uint4 *)(s_m + 4 * threadIdx.x) = gm[(int64_t)step * (F1X_MASK_WORDS / 2) + threadIdx.x];
        __syncthreads();
#pragma unroll 2
        for (int w = 0; w < F1X_STEP_WORDS; ++w) {                  // a 64-bit word (two dwords, one 8-byte LDS read each) at a time
            unsigned long long av[F1X_LDS_PLANES][2], bv[F1X_LDS_PLANES][2], mv[3];      // [plane][x or y], [class]
#pragma unroll
            for (int pl = 0; pl < F1X_LDS_PLANES; ++pl)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    av[pl][h] = *(const unsigned long long *)(s_a + (pl * F1X_TILE + i + 16 * h) * F1X_LD + 2 * w);
                    bv[pl][h] = *(const unsigned long long *)(sb + (pl * F1X_TILE + j + 16 * h) * F1X_LD + 2 * w);
                }
#pragma unroll
            for (int c = 0; c < 3; ++c) mv[c] = *(const unsigned long long *)(s_m + c * 2 * F1X_STEP_WORDS + 2 * w);
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const unsigned long long e0 = av[0][x] & bv[0][y], e1 = av[1][x] & bv[1][y];
                    const unsigned long long u = (av[2][x] & bv[2][y]) | (av[3][x] & bv[3][y]);
                    const unsigned long long ni = (av[4][x] & bv[4][y]) ^ u;
                    const unsigned long long het = ni ^ e0 ^ e1;
                    nin[x][y] += f1x_popc(ni);
                    hit[x][y] += f1x_popc((e0 & mv[0]) | (e1 & mv[1]) | (het & mv[2]));
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int a = ta * F1X_TILE + i + 16 * x;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int b = tb * F1X_TILE + j + 16 * y;
            if (a >= ncols || b >= ncols || nin[x][y] == 0) continue;      // hits <= ninfo: nothing to add either
            const int64_t ab = (int64_t)a * ncols + b, ba = (int64_t)b * ncols + a;
            atomicAdd(out_ninfo + ab, nin[x][y]);
            if (hit[x][y]) atomicAdd(out_hits + ab, hit[x][y]);
            if (!diag) {
                atomicAdd(out_ninfo + ba, nin[x][y]);
                if (hit[x][y]) atomicAdd(out_hits + ba, hit[x][y]);
            }
        }
    }
}

}  // namespace snpm
