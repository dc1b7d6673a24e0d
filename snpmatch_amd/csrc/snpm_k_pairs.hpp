// snpm_k_pairs.hpp -- pairsnp: all-pairs sample concordance (snpmatch.pairwiseScore, core/snpmatch.py:270-309 of the reference, for every pair of a cohort).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Input: one id byte per (record, sample), record-major [n, pitch] with the samples contiguous (pitch = n_samples: packed rows).  0 = the sample has no call at
// the record, 1..127 = the id of its genotype text.  Per segment (chromosome) s and pair (a, b):
//   common[s, a, b] = #records with ids[r, a] != 0 && ids[r, b] != 0
//   match [s, a, b] = #records with ids[r, a] == ids[r, b] != 0
//
// Two kernels.
//   k_pair_transpose  record-major rows -> sample-major planes [n_samples_pad, n_pad].  The record axis of the planes is cut in
//       chunks of PR_CHUNK records; every segment starts a chunk of its own and is padded with zero bytes to a whole number of
//       chunks, so no chunk holds records of two segments and the padding (id 0 = absent) adds to neither count.  Sample rows
//       past n_samples are zero.  EVERY byte of the planes is written by every call: nothing of an earlier call survives.
//   k_pair_count      grid (chunk, tile pair ta <= tb), PR_TILE x PR_TILE pairs per block, a 2 x 2 register tile of pairs per
//       lane.  The chunk is staged through LDS PR_STEP records at a time and walked a dword (4 records) at a time:
//         pa = (a + 0x7f7f7f7f) & 0x80808080      high bit of a byte set <=> the byte is not 0 (ids stop at 127: no carry)
//         ne = ((a ^ b) + 0x7f7f7f7f) & 0x80808080    ... <=> the bytes differ
//         common += popc(pa & pb),  match += popc(pa & pb & ~ne)
//       The partial counts of a chunk go into the zeroed result with int32 atomicAdd (integer sums: any order, same result);
//       a block off the diagonal of the tile grid also writes the mirrored cell.
constexpr int PR_TILE = 32;             // samples per tile side
constexpr int PR_CHUNK = 4096;          // records per block of k_pair_count; segments are padded to a multiple of it
constexpr int PR_STEP = 256;            // records staged in LDS at a time
constexpr int PR_THREADS = 256;
constexpr int PR_LD = PR_STEP / 4 + 4;  // dwords per LDS row: 272 bytes, so that rows r and r + 1 start one 16-byte slot apart
constexpr int PR_TR_SAMPLES = 64;       // k_pair_transpose: samples x records of a tile
constexpr int PR_TR_RECORDS = 256;
constexpr int PR_TR_LD = PR_TR_RECORDS + 4;     // bytes per LDS row of the transpose (65 dwords: sample rows start one bank apart)
static_assert(PR_CHUNK % PR_STEP == 0 && PR_CHUNK % PR_TR_RECORDS == 0 && PR_TR_SAMPLES % PR_TILE == 0, "whole steps and tiles per chunk");
static_assert(PR_TILE * PR_TILE == 4 * PR_THREADS, "a 2 x 2 register tile of pairs per lane");

// chunk c of the padded record axis holds chunk_cnt[c] records (1..PR_CHUNK) from row chunk_src[c] on.
// grid (chunks * PR_CHUNK / PR_TR_RECORDS, n_samples_pad / PR_TR_SAMPLES)
__global__ void __launch_bounds__(PR_THREADS)
k_pair_transpose(const uint8_t *__restrict__ ids, int64_t pitch, int n_samples, const int64_t *__restrict__ chunk_src,
                 const int32_t *__restrict__ chunk_cnt, uint8_t *__restrict__ planes, int64_t n_pad)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_t[PR_TR_SAMPLES * PR_TR_LD];     // [sample][record]
    constexpr int tiles_per_chunk = PR_CHUNK / PR_TR_RECORDS;
    const int chunk = blockIdx.x / tiles_per_chunk;
    const int rec0 = (blockIdx.x % tiles_per_chunk) * PR_TR_RECORDS;          // first record of the tile inside its chunk
    const int s0 = blockIdx.y * PR_TR_SAMPLES;
    const int64_t src = chunk_src[chunk];
    const int valid = chunk_cnt[chunk] - rec0;                                // records of this tile that exist (may be <= 0)
    // read: a wave takes the 64 samples of one record (adjacent bytes; the rows are packed, n_samples bytes each, so nothing is
    // aligned and a byte per lane it is), the block four records per pass
    const int sl = threadIdx.x & (WAVE - 1), rr = threadIdx.x >> 6;
    const bool mine = s0 + sl < n_samples;
#pragma unroll 8
    for (int r = rr; r < PR_TR_RECORDS; r += PR_THREADS / WAVE) {
        uint8_t v = 0;
        if (mine && r < valid) v = ids[(src + rec0 + r) * pitch + s0 + sl];
        s_t[sl * PR_TR_LD + r] = v;
    }
    __syncthreads();
    // write: a wave one sample row of 256 record bytes, a dword per lane
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t col = (int64_t)chunk * PR_CHUNK + rec0 + 4 * lane;
#pragma unroll 4
    for (int s = wave; s < PR_TR_SAMPLES; s += PR_THREADS / WAVE)
        *(uint32_t *)(planes + (int64_t)(s0 + s) * n_pad + col) = *(const uint32_t *)(s_t + s * PR_TR_LD + 4 * lane);
}

// grid (chunks, tile pairs): blockIdx.y counts the pairs (ta, tb) with ta <= tb row by row.  out_common / out_match
// [n_seg, n_samples, n_samples], zeroed before the launch.
__global__ void __launch_bounds__(PR_THREADS)
k_pair_count(const uint8_t *__restrict__ planes, int64_t n_pad, int n_samples, int n_tiles, const int32_t *__restrict__ chunk_seg,
             int32_t *__restrict__ out_common, int32_t *__restrict__ out_match)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_a[PR_TILE * PR_LD];
    __shared__ __attribute__((aligned(16))) uint32_t s_b[PR_TILE * PR_LD];
    const int chunk = blockIdx.x;
    int ta = 0, rest = blockIdx.y;                                  // (block-uniform) row ta of the triangle holds n_tiles - ta pairs
    while (rest >= n_tiles - ta) { rest -= n_tiles - ta; ++ta; }
    const int tb = ta + rest;
    const bool diag = ta == tb;
    const uint32_t *sb = diag ? s_a : s_b;
    // the lane's pairs: samples {i, i + 16} of tile ta against {j, j + 16} of tile tb (rows 16 apart: the 16 lanes that differ
    // in j read 16 different 16-byte slots of a bank row)
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    int com[2][2] = {{0, 0}, {0, 0}}, mat[2][2] = {{0, 0}, {0, 0}};
    const uint8_t *ga = planes + (int64_t)ta * PR_TILE * n_pad + (int64_t)chunk * PR_CHUNK;
    const uint8_t *gb = planes + (int64_t)tb * PR_TILE * n_pad + (int64_t)chunk * PR_CHUNK;
    for (int step = 0; step < PR_CHUNK / PR_STEP; ++step) {
        // stage PR_TILE rows x PR_STEP bytes of either side: 512 loads of 16 bytes, two per thread and side
#pragma unroll
        for (int k = 0; k < PR_TILE * PR_STEP / 16 / PR_THREADS; ++k) {
            const int idx = threadIdx.x + k * PR_THREADS;
            const int row = idx >> 4, slot = idx & 15;              // PR_STEP / 16 = 16 slots per row
            const int64_t off = (int64_t)row * n_pad + step * PR_STEP + 16 * slot;
            *(uint4 *)(s_a + row * PR_LD + 4 * slot) = *(const uint4 *)(ga + off);
            if (!diag) *(uint4 *)(s_b + row * PR_LD + 4 * slot) = *(const uint4 *)(gb + off);
        }
        __syncthreads();
#pragma unroll 2
        for (int slot = 0; slot < PR_STEP / 16; ++slot) {
            const uint4 a0 = *(const uint4 *)(s_a + i * PR_LD + 4 * slot);
            const uint4 a1 = *(const uint4 *)(s_a + (i + 16) * PR_LD + 4 * slot);
            const uint4 b0 = *(const uint4 *)(sb + j * PR_LD + 4 * slot);
            const uint4 b1 = *(const uint4 *)(sb + (j + 16) * PR_LD + 4 * slot);
            const uint32_t av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
            const uint32_t bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t pb[2];
#pragma unroll
                for (int y = 0; y < 2; ++y) pb[y] = (bv[y][d] + 0x7f7f7f7fu) & 0x80808080u;
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    const uint32_t pa = (av[x][d] + 0x7f7f7f7fu) & 0x80808080u;
#pragma unroll
                    for (int y = 0; y < 2; ++y) {
                        const uint32_t ne = ((av[x][d] ^ bv[y][d]) + 0x7f7f7f7fu) & 0x80808080u;
                        const uint32_t both = pa & pb[y];
                        com[x][y] += __popc(both);
                        mat[x][y] += __popc(both & ~ne);
                    }
                }
            }
        }
        __syncthreads();
    }
    const int64_t base = (int64_t)chunk_seg[chunk] * n_samples * n_samples;
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int a = ta * PR_TILE + i + 16 * x;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int b = tb * PR_TILE + j + 16 * y;
            if (a >= n_samples || b >= n_samples || com[x][y] == 0) continue;      // match <= common: nothing to add either
            const int64_t ab = base + (int64_t)a * n_samples + b, ba = base + (int64_t)b * n_samples + a;
            atomicAdd(out_common + ab, com[x][y]);
            if (mat[x][y]) atomicAdd(out_match + ab, mat[x][y]);
            if (!diag) {
                atomicAdd(out_common + ba, com[x][y]);
                if (mat[x][y]) atomicAdd(out_match + ba, mat[x][y]);
            }
        }
    }
}

}  // namespace snpm
