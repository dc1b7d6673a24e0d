// snpm_k_mk.hpp -- markers: a greedy minimal set of panel rows (SNPs) that separates every pair of accession columns `depth` times.
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp and kin_code of
// snpm_k_kin.hpp only, so that tests/mk_host_driver.cpp can compile this very text for the host (tests/host_kernel/).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Row r of the selection SEPARATES the unordered pair {a, b} of listed columns when both calls are homozygous and different: code 0
// in one column and 1 in the other.  need[a][b] (uint8, symmetric, 0 on the diagonal) starts at `depth`; a ROUND computes for every
// eligible row the number of pairs with need > 0 it separates (its gain), picks the row with the largest gain (ties: the smallest
// position), decrements the need of those pairs and makes the pick -- with `coord`, every row closer than min_dist to it as well --
// ineligible.  The textbook greedy set (multi-)cover: not optimal.  All integer, so the result is one bit pattern.
//
// The bit-planes are the other way round from the pair scans: one bit per ACCESSION, one word row per SNP.
//   k_mk_rowplanes  panel rows (int8, packed whole-row or packed split layout; a dense range or an int64 row list; a column list or
//       all columns) -> H[n_rows][2][Wc] of 64-bit words, Wc = cols_pad / 64: bit a % 64 of word a / 64 of H[r][0] is (code == 0),
//       of H[r][1] is (code == 1).  Lane = accession, so ONE wave64 ballot is a word: no transposition through LDS.  Columns past
//       ncols give zero bits.  EVERY word of H is written by every call.
//   k_mk_gain       gain[r] = sum over a in H0(r) of popcount(H1(r) & U[a]), U the symmetric bit matrix of (need > 0): every unordered
//       pair is counted once, because a is in H0 and b in H1.  U is stored word-major, Ut[w][a], so consecutive lanes (consecutive
//       a) load consecutive words; a block takes MK_GAIN_ROWS rows and all accessions: each loaded word of Ut is ANDed with that
//       word of every row's H1 (broadcast reads from LDS, [w][row] so a row group's words are one 64-byte run), popcount-accumulated,
//       masked by the lane's H0 bit of the row and reduced over the block.  A column no row of the group has in H0 is skipped.
//       Ineligible rows get gain 0 (and cost nothing once a whole group is ineligible), unless `all` asks for every row (round 0,
//       for first_gain).  A block also leaves the best of its ELIGIBLE rows as one 64-bit key, gain << 32 | (2^32 - 1 - position)
//       (0: no row with a gain): the larger key is the larger gain, then the smaller position.
//   k_mk_pick       ONE block: the largest key of the gain blocks (n_rows / MK_GAIN_ROWS words instead of every gain and eligibility
//       byte); appends the pick to chosen / gain_at, updates the 32-byte MkState, clears the eligibility of the pick and, with
//       coord, of its neighbourhood.
//   k_mk_update     one thread per cell (a, b) of need at a time, a wave per row a in steps of 64 b: tests the picked row's two bits, decrements
//       its own cell -- (a, b) and (b, a) are different threads: no atomics -- and rebuilds the words of Ut it owns by ballot.  With
//       init_depth > 0 it writes the initial need and Ut instead (the call's first launch).
// No kernel waits on another block; the rounds are plain launches in stream order (gain, pick, update).  Once MkState::done is set
// every later k_mk_gain and k_mk_pick returns at its first instruction, and so does a k_mk_update whose round made no pick.  Every
// index taken from device data (the picked position, and through it the bit words) is range-checked before use.
constexpr int MK_THREADS = 256;
constexpr int MK_PL_ROWS = 16;              // rows per block of k_mk_rowplanes (a wave takes every fourth)
constexpr int MK_GAIN_ROWS = 8;             // rows per block of k_mk_gain
constexpr int MK_PICK_THREADS = 256;        // the one block of k_mk_pick
constexpr int MK_PICK_UNROLL = 4;           // independent loads in flight per thread of k_mk_pick
constexpr int MK_MAX_WC = 64;               // words per plane row at most: 4096 accessions (SNPM_MK_MAX_ACCESSIONS)
constexpr int MK_ROUND_BATCH = 8;           // rounds the host enqueues between two reads of MkState
static_assert(MK_THREADS % WAVE == 0 && MK_PICK_THREADS % WAVE == 0 && MK_PL_ROWS % (MK_THREADS / WAVE) == 0, "whole waves; whole passes over a plane block");
static_assert(MK_GAIN_ROWS <= WAVE && MK_MAX_WC <= WAVE, "a lane per row of a gain group; lane w keeps word w of a plane row");

enum { MK_STOP_RESOLVED = 0, MK_STOP_MAX_MARKERS = 1, MK_STOP_NO_GAIN = 2 };

struct MkState {                            // 32 bytes, read by the host between batches of rounds
    long long n_chosen;                     // picks so far
    long long remaining;                    // sum of need over a < b
    long long pick;                         // position of the last pick, -1 before the first
    int32_t done;                           // the loop has ended: `reason` says why
    int32_t reason;
};
static_assert(sizeof(MkState) == 32, "the host reads 32 bytes");

// grid (ceil(n_rows / MK_PL_ROWS)).  Row r of the selection (0 <= r < n_rows) is panel row row_idx[first + r], or first + r when
// row_idx is null; column a of the call (0 <= a < ncols) is panel column cols[a], or a when cols is null.  Wc <= MK_MAX_WC.
__global__ void __launch_bounds__(MK_THREADS)
k_mk_rowplanes(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, const int64_t *__restrict__ row_idx, int64_t first, int64_t n_rows,
               const int32_t *__restrict__ cols, int ncols, unsigned long long *__restrict__ H, int Wc)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * MK_PL_ROWS;
    for (int k = wave; k < MK_PL_ROWS; k += MK_THREADS / WAVE) {
        const int64_t r = r0 + k;
        if (r >= n_rows) break;                                      // (wave-uniform)
        const int64_t prow = row_idx ? row_idx[first + r] : first + r;
        unsigned long long k0 = 0ull, k1 = 0ull;                    // lane w keeps the two words w of the row
        for (int w = 0; w < Wc; ++w) {
            const int c = w * WAVE + lane;
            uint32_t v = 0xFFu;
            if (c < ncols) v = kin_code(db, pitch, desc, prow, cols ? (int64_t)cols[c] : (int64_t)c);
            const unsigned long long b0 = __ballot(v == 0u), b1 = __ballot(v == 1u);
            if (lane == w) { k0 = b0; k1 = b1; }
        }
        if (lane < Wc) {
            H[(r * 2) * Wc + lane] = k0;
            H[(r * 2 + 1) * Wc + lane] = k1;
        }
    }
}

// a block's best row as a key (see above); n_rows < 2^31
__host__ __device__ __forceinline__ unsigned long long mk_key(int32_t gain, int64_t pos)
{
    return (unsigned long long)(uint32_t)gain << 32 | (unsigned long long)(0xFFFFFFFFu - (uint32_t)pos);
}

// grid (ceil(n_rows / MK_GAIN_ROWS)).  Ut [Wc][cols_pad]; elig [n_rows] (0: not eligible); gain [n_rows]; best [gridDim.x].
__global__ void __launch_bounds__(MK_THREADS)
k_mk_gain(const unsigned long long *__restrict__ H, const unsigned long long *__restrict__ Ut, const uint8_t *__restrict__ elig,
          const MkState *__restrict__ st, int64_t n_rows, int64_t cols_pad, int Wc, int all, int32_t *__restrict__ gain,
          unsigned long long *__restrict__ best)
{
    if (st->done) return;
    __shared__ __attribute__((aligned(16))) unsigned long long s_h1[MK_MAX_WC * MK_GAIN_ROWS];     // [word][row of the group]
    __shared__ __attribute__((aligned(16))) unsigned long long s_h0[MK_GAIN_ROWS * MK_MAX_WC];     // [row of the group][word]
    __shared__ int32_t s_red[MK_THREADS / WAVE][MK_GAIN_ROWS];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * MK_GAIN_ROWS;
    uint32_t live = 0, may = 0;                                      // (block-uniform) rows of the group that get a gain / that may be picked
#pragma unroll
    for (int g = 0; g < MK_GAIN_ROWS; ++g)
        if (r0 + g < n_rows) {
            if (elig[r0 + g]) may |= 1u << g;
            if (all || (may >> g & 1u)) live |= 1u << g;
        }
    if (!live) {
        if ((int)threadIdx.x < MK_GAIN_ROWS && r0 + (int)threadIdx.x < n_rows) gain[r0 + threadIdx.x] = 0;
        if (threadIdx.x == 0) best[blockIdx.x] = 0ull;
        return;
    }
    for (int i = threadIdx.x; i < MK_GAIN_ROWS * Wc; i += MK_THREADS) {
        const int g = i / Wc, w = i - g * Wc;
        const bool on = live >> g & 1u;
        s_h0[g * MK_MAX_WC + w] = on ? H[((r0 + g) * 2) * Wc + w] : 0ull;
        s_h1[w * MK_GAIN_ROWS + g] = on ? H[((r0 + g) * 2 + 1) * Wc + w] : 0ull;
    }
    __syncthreads();
    int32_t tot[MK_GAIN_ROWS];
#pragma unroll
    for (int g = 0; g < MK_GAIN_ROWS; ++g) tot[g] = 0;
    for (int64_t a = threadIdx.x; a < cols_pad; a += MK_THREADS) {
        uint32_t in0 = 0;                                            // bit g: accession a is in H0 of row g
#pragma unroll
        for (int g = 0; g < MK_GAIN_ROWS; ++g) in0 |= (uint32_t)(s_h0[g * MK_MAX_WC + (int)(a >> 6)] >> (a & 63) & 1ull) << g;
        if (!in0) continue;
        int32_t acc[MK_GAIN_ROWS];
#pragma unroll
        for (int g = 0; g < MK_GAIN_ROWS; ++g) acc[g] = 0;
        for (int w = 0; w < Wc; ++w) {
            const unsigned long long u = Ut[(int64_t)w * cols_pad + a];
            const uint32_t ulo = (uint32_t)u, uhi = (uint32_t)(u >> 32);
#pragma unroll
            for (int g = 0; g < MK_GAIN_ROWS; ++g) {
                const unsigned long long h = s_h1[w * MK_GAIN_ROWS + g];
                acc[g] += __popc(ulo & (uint32_t)h) + __popc(uhi & (uint32_t)(h >> 32));
            }
        }
#pragma unroll
        for (int g = 0; g < MK_GAIN_ROWS; ++g) tot[g] += (in0 >> g & 1u) ? acc[g] : 0;
    }
#pragma unroll
    for (int g = 0; g < MK_GAIN_ROWS; ++g) {
        uint32_t v = (uint32_t)tot[g];
        for (int m = WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m);
        if (lane == 0) s_red[wave][g] = (int32_t)v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long key = 0ull;
        for (int g = 0; g < MK_GAIN_ROWS && r0 + g < n_rows; ++g) {
            int32_t sum = 0;
#pragma unroll
            for (int k = 0; k < MK_THREADS / WAVE; ++k) sum += s_red[k][g];
            gain[r0 + g] = sum;                                     // (a row that is not live has zero planes: 0)
            if ((may >> g & 1u) && sum > 0 && mk_key(sum, r0 + g) > key) key = mk_key(sum, r0 + g);
        }
        best[blockIdx.x] = key;
    }
}

// |x - y| of two int64 values, exact: the difference is taken in uint64
__host__ __device__ __forceinline__ unsigned long long mk_dist(int64_t x, int64_t y)
{
    return x > y ? (unsigned long long)x - (unsigned long long)y : (unsigned long long)y - (unsigned long long)x;
}

// grid (1), MK_PICK_THREADS threads.  best [n_best]: the keys of the n_best blocks of this round's k_mk_gain.  chosen / gain_at hold
// `cap` entries (the host's bound on the rounds, <= max_markers); coord null: no neighbourhood.
__global__ void __launch_bounds__(MK_PICK_THREADS)
k_mk_pick(const unsigned long long *__restrict__ best, int64_t n_best, uint8_t *__restrict__ elig, const int64_t *__restrict__ coord, int64_t min_dist,
          int64_t n_rows, int64_t max_markers, int64_t cap, int64_t *__restrict__ chosen, int32_t *__restrict__ gain_at, MkState *__restrict__ st)
{
    if (st->done) return;                                            // (read by every thread before the first barrier; written behind it)
    __shared__ unsigned long long s_key[MK_PICK_THREADS / WAVE];
    __shared__ long long s_pick;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    unsigned long long key = 0ull;
    for (int64_t i = threadIdx.x; i < n_best; i += MK_PICK_THREADS * MK_PICK_UNROLL) {
        unsigned long long k[MK_PICK_UNROLL];
#pragma unroll
        for (int u = 0; u < MK_PICK_UNROLL; ++u) k[u] = i + u * MK_PICK_THREADS < n_best ? best[i + u * MK_PICK_THREADS] : 0ull;
#pragma unroll
        for (int u = 0; u < MK_PICK_UNROLL; ++u) key = k[u] > key ? k[u] : key;
    }
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((uint32_t)(key >> 32), m) << 32 | __shfl_xor((uint32_t)key, m);
        key = o > key ? o : key;
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < MK_PICK_THREADS / WAVE; ++k) key = s_key[k] > key ? s_key[k] : key;
        const uint32_t bg = (uint32_t)(key >> 32);                   // the best gain (0: no eligible row has one) and its position
        const int64_t bp = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
        const long long n = st->n_chosen;
        long long pick = -1;
        if (st->remaining <= 0) { st->done = 1; st->reason = MK_STOP_RESOLVED; }
        else if (n >= max_markers) { st->done = 1; st->reason = MK_STOP_MAX_MARKERS; }
        else if (bg == 0 || bg > 0x7FFFFFFFu || bp >= n_rows || n < 0 || n >= cap) { st->done = 1; st->reason = MK_STOP_NO_GAIN; }
        else {
            pick = (long long)bp;
            chosen[n] = pick;
            gain_at[n] = (int32_t)bg;
            elig[pick] = 0;
            st->n_chosen = n + 1;
            st->remaining -= (long long)bg;
            st->pick = pick;
            if (st->remaining <= 0) { st->done = 1; st->reason = MK_STOP_RESOLVED; }
            else if (n + 1 >= max_markers) { st->done = 1; st->reason = MK_STOP_MAX_MARKERS; }
        }
        s_pick = pick;
    }
    __syncthreads();
    const long long pick = s_pick;
    if (pick < 0 || !coord || min_dist <= 0) return;                 // (block-uniform)
    const int64_t c0 = coord[pick];
    for (int64_t r = threadIdx.x; r < n_rows; r += MK_PICK_THREADS * MK_PICK_UNROLL) {
        int64_t c[MK_PICK_UNROLL];
#pragma unroll
        for (int u = 0; u < MK_PICK_UNROLL; ++u) c[u] = r + u * MK_PICK_THREADS < n_rows ? coord[r + u * MK_PICK_THREADS] : c0;
#pragma unroll
        for (int u = 0; u < MK_PICK_UNROLL; ++u)
            if (r + u * MK_PICK_THREADS < n_rows && mk_dist(c[u], c0) < (unsigned long long)min_dist) elig[r + u * MK_PICK_THREADS] = 0;
    }
}

// grid (cols_pad / (MK_THREADS / WAVE)): wave a owns row a of need [ncols][ncols], 64 cells per step, and the words Ut[.][a].
// `round` is the index of the round this launch belongs to: the round picked a row iff n_chosen == round + 1.
__global__ void __launch_bounds__(MK_THREADS)
k_mk_update(const unsigned long long *__restrict__ H, int64_t n_rows, int Wc, int ncols, int64_t cols_pad, const MkState *__restrict__ st,
            int64_t round, int init_depth, uint8_t *__restrict__ need, unsigned long long *__restrict__ Ut)
{
    long long pos = -1;
    if (!init_depth) {
        if (st->n_chosen != round + 1) return;                       // this round picked nothing: need and Ut stand
        pos = st->pick;
        if (pos < 0 || pos >= n_rows) return;
    }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t a = (int64_t)blockIdx.x * (MK_THREADS / WAVE) + wave;
    if (a >= cols_pad) return;                                       // (a grid of whole blocks never gets here)
    const unsigned long long *h0 = H + (init_depth ? 0 : pos * 2) * Wc, *h1 = h0 + Wc;      // (not read when init_depth)
    uint32_t a0 = 0, a1 = 0;
    if (!init_depth) {
        a0 = (uint32_t)(h0[a >> 6] >> (a & 63) & 1ull);
        a1 = (uint32_t)(h1[a >> 6] >> (a & 63) & 1ull);
        if (!(a0 | a1)) return;                                      // (wave-uniform) the pick separates a from nobody: row a of need stands
    }
    for (int w = 0; w < Wc; ++w) {
        const int64_t b = (int64_t)w * WAVE + lane;
        uint32_t n = 0;
        if (a < ncols && b < ncols) {
            uint8_t *cell = need + a * ncols + b;
            if (init_depth) {
                n = a != b ? (uint32_t)init_depth : 0u;
                *cell = (uint8_t)n;
            } else {
                const uint32_t b0 = (uint32_t)(h0[w] >> lane & 1ull), b1 = (uint32_t)(h1[w] >> lane & 1ull);
                n = *cell;
                if (n && ((a0 & b1) | (a1 & b0))) *cell = (uint8_t)--n;
            }
        }
        const unsigned long long open = __ballot(n > 0u);
        if (lane == 0) Ut[(int64_t)w * cols_pad + a] = open;
    }
}

}  // namespace snpm
