// snpm_k_kin.hpp -- panel kinship: all-pairs accession relatedness over panel rows (Genotype.kinship_given_snps / calc_kinship_mat, core/snp_genotype.py:256-289, :440-459 of the reference).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs pk_off / WAVE of snpm_k_common.hpp only, so
// that tests/kin_host_driver.cpp can compile this very text for the host (tests/host_kernel/).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Per pair (a, b) of listed accession columns over the listed panel rows, three int32 counts:
//   ninfo[a, b] = #rows where both calls are not missing (hets and the int8 panel's "other" code 3 included)
//   same [a, b] = #rows where both calls are homozygous (0 or 1) and equal
//   diff [a, b] = #rows where both calls are homozygous and different
// The reference's kinship is (same - diff) / ninfo.
//
// Two kernels, run once per SLAB of rows (the host cuts the row axis so that the planes fit a workspace budget):
//   k_kin_planes  panel rows (int8, packed whole-row or packed split layout; a dense range or an int64 row list; a column list or
//       all columns) -> accession-major bit-planes [3][cols_pad][W] of 64-bit words, one bit per row: P0 = (v == 0), P1 = (v == 1),
//       I = (v not missing).  A block takes 64 rows x 64 accessions: the canonical codes go through LDS (read with lane = accession:
//       per wave 64 adjacent bytes of an int8 row, 16 of a packed one), then with lane = row three wave64 ballots per accession
//       ARE the three words.  Rows past the
//       slab's end (W is padded to whole LDS steps of the count kernel) and accessions past ncols give zero bits in all three planes,
//       so they add to no count.  EVERY word of [3][cols_pad][W] is written by every launch: nothing of an earlier slab or call
//       survives.
//   k_kin_count   grid (tile pair ta <= tb, chunk of KN_CHUNK_WORDS words), KN_TILE x KN_TILE pairs per block, a 2 x 2 register tile
//       of pairs per lane.  The three planes of either side are staged through LDS KN_STEP_WORDS words at a time (a block on the
//       diagonal stages one side) and walked a dword at a time:
//         ninfo += popc(Ia & Ib),  same += popc(P0a & P0b) + popc(P1a & P1b),  diff += popc(P0a & P1b) + popc(P1a & P0b)
//       i.e. 5 AND + 5 popcount-accumulate per pair and dword: 20 32-bit VALU operations per pair and 64 rows.  The partial counts
//       of a chunk go into the zeroed results with int32 atomicAdd (integer sums: any order, same result; zero partials are
//       skipped); a block off the diagonal also writes the mirrored cell.  The tile pair is the FAST grid axis: the blocks in
//       flight share one chunk, whose planes (3 KiB per accession) stay in L2.
constexpr int KN_TILE = 32;                 // accessions per tile side of k_kin_count
constexpr int KN_THREADS = 256;
constexpr int KN_STEP_WORDS = 16;           // 64-bit words (= 1024 rows, 128 B per plane row) staged in LDS at a time; W is a multiple of it
constexpr int KN_CHUNK_WORDS = 128;         // words (= 8192 rows) per block of k_kin_count
constexpr int KN_LD = KN_STEP_WORDS * 2 + 4;    // dwords per LDS row: 144 bytes = 9 slots of 16 bytes, rows r and r + 1 start one slot (mod 16: nine) apart
constexpr int KN_PL_ROWS = 64;              // k_kin_planes: rows x accessions of a tile
constexpr int KN_PL_COLS = 64;
constexpr int KN_PL_LD = KN_PL_COLS + 4;    // bytes per LDS row of the tile (17 dwords: the 64 rows a wave reads start in different banks)
static_assert(KN_CHUNK_WORDS % KN_STEP_WORDS == 0 && KN_PL_COLS % KN_TILE == 0 && KN_PL_ROWS == WAVE, "whole steps per chunk, whole count tiles per plane tile, a ballot is a word");
static_assert(KN_TILE * KN_TILE == 4 * KN_THREADS, "a 2 x 2 register tile of pairs per lane");
static_assert(KN_TILE * KN_STEP_WORDS * 8 / 16 == KN_THREADS, "one 16-byte load per thread, plane and side of a step");

// The host's slab plan: LDS steps (KN_STEP_ROWS rows each) of one slab of an n_rows scan whose planes [3][cols_pad][W] must fit
// ws_bytes -- whole chunks where the budget holds one, at least one step, at most 65535 chunks (grid.y of k_kin_count) and no more
// than the rows need.  A slab's planes take kin_slab_steps(..) * kin_step_bytes(cols_pad) bytes.
constexpr int64_t KN_STEP_ROWS = (int64_t)KN_STEP_WORDS * 64;
__host__ __device__ __forceinline__ int64_t kin_step_bytes(int64_t cols_pad) { return 3 * cols_pad * KN_STEP_WORDS * 8; }
__host__ __device__ __forceinline__ int64_t kin_slab_steps(size_t ws_bytes, int64_t cols_pad, int64_t n_rows)
{
    const int64_t steps_per_chunk = KN_CHUNK_WORDS / KN_STEP_WORDS, need = (n_rows + KN_STEP_ROWS - 1) / KN_STEP_ROWS;
    int64_t steps = (int64_t)(ws_bytes / (size_t)kin_step_bytes(cols_pad));
    if (steps < 1) steps = 1;
    if (steps >= steps_per_chunk) steps = steps / steps_per_chunk * steps_per_chunk;
    if (steps > 65535 * steps_per_chunk) steps = 65535 * steps_per_chunk;
    return steps < need ? steps : need;
}

// canonical code of (row, accession): 0 ref, 1 alt, 2 het, 3 other (int8 panels), 0xFF missing.  `desc` is the panel's layout
// descriptor (snpm_k_common.hpp): 0 = int8 rows of `pitch` bytes, else 2-bit fields in whole or split rows.
__device__ __forceinline__ uint32_t kin_code(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, int64_t prow, int64_t col)
{
    if (desc) {
        const uint32_t v = (uint32_t)(((const uint8_t *)db)[pk_off(pitch, desc, prow, col >> 2)] >> (2 * (int)(col & 3))) & 3u;
        return v == 3u ? 0xFFu : v;
    }
    const int v = db[prow * pitch + col];
    return v < 0 ? 0xFFu : (uint32_t)v;
}

// grid (W, cols_pad / KN_PL_COLS).  Row k of the slab (0 <= k < n_valid) is panel row
// row_idx[first + k], or first + k when row_idx is null; column a of the call (0 <= a < ncols) is panel column cols[a], or a when
// cols is null.
__global__ void __launch_bounds__(KN_THREADS)
k_kin_planes(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, const int64_t *__restrict__ row_idx, int64_t first, int64_t n_valid,
             const int32_t *__restrict__ cols, int ncols, unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_c[KN_PL_ROWS * KN_PL_LD];       // [row][accession]
    const int64_t word = blockIdx.x;
    const int c0 = blockIdx.y * KN_PL_COLS;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t r0 = word * KN_PL_ROWS;
    const int64_t plane = cols_pad * W;
    if (r0 >= n_valid) {                    // (block-uniform) a word of padding rows only
        if (threadIdx.x < KN_PL_COLS) {
            const int64_t at = (int64_t)(c0 + (int)threadIdx.x) * W + word;
            planes[at] = 0ull;
            planes[plane + at] = 0ull;
            planes[2 * plane + at] = 0ull;
        }
        return;
    }
    // read: a wave takes the 64 accessions of one row, the block four rows per pass
    const bool have = c0 + lane < ncols;
    const int64_t col = have ? (cols ? (int64_t)cols[c0 + lane] : (int64_t)(c0 + lane)) : 0;
#pragma unroll 4
    for (int r = wave; r < KN_PL_ROWS; r += KN_THREADS / WAVE) {
        uint32_t v = 0xFFu;
        if (have && r0 + r < n_valid) {
            const int64_t prow = row_idx ? row_idx[first + r0 + r] : first + r0 + r;
            v = kin_code(db, pitch, desc, prow, col);
        }
        s_c[r * KN_PL_LD + lane] = (uint8_t)v;
    }
    __syncthreads();
    // lane = row: a wave takes 16 accessions; lane k keeps the three words of the wave's accession k
    constexpr int per_wave = KN_PL_COLS / (KN_THREADS / WAVE);
    unsigned long long k0 = 0ull, k1 = 0ull, ki = 0ull;
#pragma unroll 4
    for (int k = 0; k < per_wave; ++k) {
        const uint32_t v = s_c[lane * KN_PL_LD + wave * per_wave + k];
        const unsigned long long b0 = __ballot(v == 0u), b1 = __ballot(v == 1u), bi = __ballot(v != 0xFFu);
        if (lane == k) { k0 = b0; k1 = b1; ki = bi; }
    }
    if (lane < per_wave) {
        const int64_t at = (int64_t)(c0 + wave * per_wave + lane) * W + word;
        planes[at] = k0;
        planes[plane + at] = k1;
        planes[2 * plane + at] = ki;
    }
}

// grid (tile pairs, chunks): blockIdx.x counts the pairs (ta, tb) with ta <= tb row by row.  out_* [ncols, ncols], zeroed before the
// first slab.  W (words per plane row of this slab) is a multiple of KN_STEP_WORDS; the last chunk may hold fewer steps.
__global__ void __launch_bounds__(KN_THREADS)
k_kin_count(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, int ncols, int n_tiles,
            int32_t *__restrict__ out_ninfo, int32_t *__restrict__ out_same, int32_t *__restrict__ out_diff)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_a[3 * KN_TILE * KN_LD];      // [plane][accession][dword]
    __shared__ __attribute__((aligned(16))) uint32_t s_b[3 * KN_TILE * KN_LD];
    int ta = 0, rest = blockIdx.x;                                  // (block-uniform) row ta of the triangle holds n_tiles - ta pairs
    while (rest >= n_tiles - ta) { rest -= n_tiles - ta; ++ta; }
    const int tb = ta + rest;
    const bool diag = ta == tb;
    const uint32_t *sb = diag ? s_a : s_b;
    const int64_t w0 = (int64_t)blockIdx.y * KN_CHUNK_WORDS;
    const int64_t left = (W - w0) / KN_STEP_WORDS;
    const int steps = (int)(left < KN_CHUNK_WORDS / KN_STEP_WORDS ? left : KN_CHUNK_WORDS / KN_STEP_WORDS);
    // the lane's pairs: accessions {i, i + 16} of tile ta against {j, j + 16} of tile tb (the 16 lanes that differ in j read 16
    // different 16-byte slots; the 4 values of i in a wave are broadcasts)
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    int nin[2][2] = {{0, 0}, {0, 0}}, sam[2][2] = {{0, 0}, {0, 0}}, dif[2][2] = {{0, 0}, {0, 0}};
    const int64_t row_bytes = W * 8, plane_bytes = cols_pad * row_bytes;
    const uint8_t *base = (const uint8_t *)planes;
    const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;      // staging: one 16-byte slot of one accession per plane and side
    const int64_t ga = (int64_t)(ta * KN_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const int64_t gb = (int64_t)(tb * KN_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    for (int step = 0; step < steps; ++step) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const int64_t off = pl * plane_bytes + (int64_t)step * (KN_STEP_WORDS * 8);
            *(uint4 *)(s_a + (pl * KN_TILE + srow) * KN_LD + 4 * sslot) = *(const uint4 *)(base + ga + off);
            if (!diag) *(uint4 *)(s_b + (pl * KN_TILE + srow) * KN_LD + 4 * sslot) = *(const uint4 *)(base + gb + off);
        }
        __syncthreads();
#pragma unroll 2
        for (int slot = 0; slot < KN_STEP_WORDS / 2; ++slot) {
            uint32_t av[3][2][4], bv[3][2][4];                      // [plane][x or y][dword]
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint4 a = *(const uint4 *)(s_a + (pl * KN_TILE + i + 16 * h) * KN_LD + 4 * slot);
                    const uint4 b = *(const uint4 *)(sb + (pl * KN_TILE + j + 16 * h) * KN_LD + 4 * slot);
                    av[pl][h][0] = a.x; av[pl][h][1] = a.y; av[pl][h][2] = a.z; av[pl][h][3] = a.w;
                    bv[pl][h][0] = b.x; bv[pl][h][1] = b.y; bv[pl][h][2] = b.z; bv[pl][h][3] = b.w;
                }
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) {
                        nin[x][y] += __popc(av[2][x][d] & bv[2][y][d]);
                        sam[x][y] += __popc(av[0][x][d] & bv[0][y][d]) + __popc(av[1][x][d] & bv[1][y][d]);
                        dif[x][y] += __popc(av[0][x][d] & bv[1][y][d]) + __popc(av[1][x][d] & bv[0][y][d]);
                    }
        }
        __syncthreads();
    }
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int a = ta * KN_TILE + i + 16 * x;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int b = tb * KN_TILE + j + 16 * y;
            if (a >= ncols || b >= ncols || nin[x][y] == 0) continue;      // same + diff <= ninfo: nothing to add either
            const int64_t ab = (int64_t)a * ncols + b, ba = (int64_t)b * ncols + a;
            atomicAdd(out_ninfo + ab, nin[x][y]);
            if (sam[x][y]) atomicAdd(out_same + ab, sam[x][y]);
            if (dif[x][y]) atomicAdd(out_diff + ab, dif[x][y]);
            if (!diag) {
                atomicAdd(out_ninfo + ba, nin[x][y]);
                if (sam[x][y]) atomicAdd(out_same + ba, sam[x][y]);
                if (dif[x][y]) atomicAdd(out_diff + ba, dif[x][y]);
            }
        }
    }
}

}  // namespace snpm
