// snpm_k_adm.hpp -- admixture: one joint EM iteration of the model of STRUCTURE / FRAPPE / ADMIXTURE on the accession columns of the resident panel -- every accession a mixture of K ancestral populations, every population with its own alt frequency at every row.  The package's own command: the reference has no counterpart.
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp, kin_code of
// snpm_k_kin.hpp and pca_shfl_xor of snpm_k_pca.hpp only, so that tests/adm_host_driver.cpp can compile this very text for the host
// (tests/host_kernel/).
#pragma once

#ifndef SNPM_ADMIX_MAX_K
#define SNPM_ADMIX_MAX_K 16                 // (include/snpmatch_hip.h carries the same figures for callers)
#endif
#ifndef SNPM_ADMIX_EPS
#define SNPM_ADMIX_EPS 1e-6
#endif

namespace snpm {
// ------------------------------------------------------------------------------------------------
// THE MODEL (include/snpmatch_hip.h has the contract).  Q [ncols][K]: the ancestry of every listed column, rows summing to 1; F
// [n_rows][K]: the alt frequency of every component at every selected row, inside [EPS, 1 - EPS].  The dosage g of a call is 0
// (ref), 2 (alt), 1 (het); a missing call and an int8 panel's "other" code are NO CALL: the cell contributes nothing anywhere.  For
// a called cell (s, i), k ascending, fma:  p = sum_k q_ik f_sk,  pbar = sum_k q_ik (1 - f_sk)  (its own positive sum, never 1 - p),
//   u = g / p,  v = (2 - g) / pbar,  ll += [g > 0] g ln p + [g < 2] (2 - g) ln pbar
//   a_sk = sum_i u q_ik,  b_sk = sum_i v q_ik,  c_ik = sum_s (u f_sk + v (1 - f_sk))
//   f'_sk = clamp(f a / (f a + (1 - f) b), EPS, 1 - EPS), unchanged where the denominator is 0
//   w_ik = q_ik c_ik,  q'_ik = w_ik / sum_k w_ik, unchanged where that sum is 0
// Both (Q', F') are made from the OLD pair: joint EM, the likelihood never decreases.  A homozygous call has one of u, v zero
// (0 / x is 0 exactly), so its cell takes ONE division and ONE logarithm; a het call two of each (adm_ratios, adm_loglik).
//
// All arithmetic is fp64, `/` is the IEEE division (-ffp-contract=off, no fast-math), fma is explicit; no floating-point atomic:
// every output has one owner and one order of summation, a function of (n_rows, ncols, K) alone -- no grid is sized by the device.
//
// K goes in steps KT = 4 / 8 / 16 (adm_pitch): the device copies of Q and F have rows of KT doubles, the entries at and beyond K
// zero.  A padded component has q = 0, so it adds fma(0, f, p) = p to the sums of a cell, a = b = 0 to its row (the denominator
// is 0: unchanged) and w = 0 to its column: the K real components get the bits they would get without the padding.
//
// k_adm_rows<KT>: a wave per selected row, the scheme of k_pca_load: lane l takes listed columns l, l + 64, ..., reads the call with
//   kin_code, the column's row of Q from global memory (Q is ncols x KT x 8 bytes, 73 KB at 1135 x 8: every wave of the grid reads
//   the same rows, they stay in L2), holds the row's KT frequencies, and accumulates a[KT], b[KT] and its share of ll, statically
//   indexed.  The halving exchange of k_pca_load sums the lanes (adm_wave_sum: log2 KT halving steps leave component lane >> (6 -
//   log2 KT) in every lane, the butterfly steps that remain sum it over the lanes that share it).  The owner lane of component k
//   writes F'[s][k]; ll is summed over the lanes by a six-step butterfly.  A wave takes ADM_ROWS_PER_WAVE consecutive rows and adds
//   their ll in row order, the block adds its four waves in wave order and stores ll_blk[block]: ADM_ROWS_PER_BLOCK rows per entry.
// k_adm_cols<KT>: a thread per listed column.  A block is ADM_COLS_THREADS consecutive listed columns times a contiguous run of the
//   selected rows (a split: adm_split_rows rows each, a function of (n_rows, ncols) alone).  The rows of a run go through LDS
//   ADM_CHUNK_ROWS at a time -- panel row index and the KT frequencies, block-uniform, read as broadcasts -- c[KT] and the column's q
//   stay in registers; an int8 row is 256 consecutive bytes per block.  The block STORES part[split][column][KT]: one writer per cell.
// k_adm_fold<KT>: blocks 0 .. n - 2, a thread per listed column and component, add the splits in order, form w, normalise (the w of
//   a column meet in LDS; each of its threads adds them k ascending), write Q'.  The LAST
//   block reduces ll_blk to the one number of the iteration in a fixed tree of radix ADM_TREE_RADIX: every level adds four
//   neighbours in order into the other of two buffers.  Depth of the likelihood sum: the lane's run (ceil(ncols / 64) cells), 6
//   butterfly steps, 7 + 3 additions in the block, 3 per tree level and at most 13 levels (n_rows < 2^31): 55 beside the run.
constexpr int ADM_ROWS_THREADS = 256;
constexpr int ADM_ROWS_PER_WAVE = 8;
constexpr int ADM_ROWS_PER_BLOCK = ADM_ROWS_THREADS / WAVE * ADM_ROWS_PER_WAVE;     // rows per entry of ll_blk
constexpr int ADM_COLS_THREADS = 256;       // listed columns per block of k_adm_cols
constexpr int ADM_CHUNK_ROWS = 16;          // rows of a run staged in LDS at a time
constexpr int ADM_SPLIT_MIN_ROWS = 16;      // a split is never shorter (but for the last one)
constexpr int ADM_BLOCKS_WANTED = 512;      // two blocks per CU of a 256-CU device
constexpr int ADM_FOLD_THREADS = 1024;
constexpr int ADM_TREE_RADIX = 4;
static_assert(SNPM_ADMIX_MAX_K <= WAVE, "one owner lane per component");
static_assert(ADM_FOLD_THREADS % SNPM_ADMIX_MAX_K == 0, "whole columns per block of k_adm_fold");

// doubles per row of the device copies of Q, F and of the partials
__host__ __device__ __forceinline__ int adm_pitch(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : 16; }

// rows per split of k_adm_cols: enough splits for ADM_BLOCKS_WANTED blocks at this width, no split below ADM_SPLIT_MIN_ROWS rows
__host__ __device__ __forceinline__ int64_t adm_split_rows(int64_t n_rows, int64_t ncols)
{
    const int64_t col_blocks = (ncols + ADM_COLS_THREADS - 1) / ADM_COLS_THREADS;
    const int64_t wanted = (ADM_BLOCKS_WANTED + col_blocks - 1) / col_blocks;
    const int64_t per = (n_rows + wanted - 1) / wanted;
    return per < ADM_SPLIT_MIN_ROWS ? ADM_SPLIT_MIN_ROWS : per;
}
__host__ __device__ __forceinline__ int64_t adm_splits(int64_t n_rows, int64_t ncols)
{
    const int64_t per = adm_split_rows(n_rows, ncols);
    return (n_rows + per - 1) / per;
}
// entries of ll_blk, and of the second buffer of the tree
__host__ __device__ __forceinline__ int64_t adm_ll_blocks(int64_t n_rows) { return (n_rows + ADM_ROWS_PER_BLOCK - 1) / ADM_ROWS_PER_BLOCK; }

// column blocks of k_adm_fold: ADM_FOLD_THREADS / KT whole columns each
__host__ __device__ __forceinline__ int64_t adm_fold_col_blocks(int64_t ncols, int kt) { return (ncols * kt + ADM_FOLD_THREADS - 1) / ADM_FOLD_THREADS; }

constexpr int adm_log2(int n) { return n <= 1 ? 0 : 1 + adm_log2(n / 2); }

// p and pbar of a cell: k ascending, fma; fb[k] = 1 - f[k]
template <int KT>
__device__ __forceinline__ void adm_mix(const double *q, const double *f, const double *fb, double &p, double &pbar)
{
    p = 0.0;
    pbar = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        p = fma(q[k], f[k], p);
        pbar = fma(q[k], fb[k], pbar);
    }
}

// u = g / p and v = (2 - g) / pbar of a called cell (code 0 ref: g = 0, 1 alt: g = 2, 2 het: g = 1)
__device__ __forceinline__ void adm_ratios(uint32_t code, double p, double pbar, double &u, double &v)
{
    if (code == 2u) {
        u = 1.0 / p;
        v = 1.0 / pbar;
    } else {
        const double d = 2.0 / (code == 1u ? p : pbar);
        u = code == 1u ? d : 0.0;
        v = code == 1u ? 0.0 : d;
    }
}

// [g > 0] g ln p + [g < 2] (2 - g) ln pbar
__device__ __forceinline__ double adm_loglik(uint32_t code, double p, double pbar)
{
    if (code == 2u) return log(p) + log(pbar);
    return 2.0 * log(code == 1u ? p : pbar);
}

// the lanes' sums of r[0 .. KT): every lane returns component lane >> (6 - log2 KT), summed over the wave (k_pca_load's exchange:
// at distance o the lanes with (lane & o) set keep the upper half of their components and send the lower, the others the other way
// round; then one component is left per lane and the remaining distances are plain butterfly steps)
// (N components in r, the next distance O: a recursion over the template arguments, so that every index is a constant -- as a loop
// over the steps the array was indexed dynamically, a chain of selects per component, and the kernel spilled scalar registers)
template <int N, int O>
__device__ __forceinline__ double adm_wave_sum(const double *r, int lane)
{
    if constexpr (N == 1) {
        double sum = r[0];
#pragma unroll
        for (int o = O; o >= 1; o >>= 1) sum += pca_shfl_xor(sum, o);
        return sum;
    } else {
        double h[N / 2];
        const bool up = (lane & O) != 0;
#pragma unroll
        for (int c = 0; c < N / 2; ++c) {
            const double keep = up ? r[c + N / 2] : r[c], send = up ? r[c] : r[c + N / 2];
            h[c] = keep + pca_shfl_xor(send, O);
        }
        return adm_wave_sum<N / 2, O / 2>(h, lane);
    }
}

// grid (ceil(n_rows / ADM_ROWS_PER_BLOCK)).  Row s of the selection (0 <= s < n_rows) is panel row row_idx[first + s], or first + s
// when row_idx is null; column a of the call (0 <= a < ncols) is panel column cols[a], or a when cols is null.  Q [ncols][KT], F and
// F_new [n_rows][KT], 1 <= K <= KT; F_new[s][k] is written for k < K when update_f is set (the entries beyond K keep the zeros
// the host put there); ll_blk [gridDim.x]: every entry is written.
template <int KT>
__global__ void __launch_bounds__(ADM_ROWS_THREADS)
k_adm_rows(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, const int64_t *__restrict__ row_idx, int64_t first, int64_t n_rows,
           const int32_t *__restrict__ cols, int64_t ncols, const double *__restrict__ Q, const double *__restrict__ F, int K, int update_f,
           double *__restrict__ F_new, double *__restrict__ ll_blk)
{
    constexpr int waves = ADM_ROWS_THREADS / WAVE, sh = 6 - adm_log2(KT);
    __shared__ double s_ll[waves];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int64_t s_base = ((int64_t)blockIdx.x * waves + wave) * ADM_ROWS_PER_WAVE;
    double ll_wave = 0.0;
#pragma unroll 1
    for (int j = 0; j < ADM_ROWS_PER_WAVE; ++j) {
        const int64_t s = s_base + j;
        if (s >= n_rows) break;                                      // (wave-uniform)
        const int64_t prow = row_idx ? row_idx[first + s] : first + s;
        double f[KT], fb[KT], a[KT], b[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            f[k] = F[s * KT + k];
            fb[k] = 1.0 - f[k];
            a[k] = 0.0;
            b[k] = 0.0;
        }
        double ll = 0.0;
        for (int64_t c = lane; c < ncols; c += WAVE) {
            const int64_t col = cols ? (int64_t)cols[c] : c;
            const uint32_t code = kin_code(db, pitch, desc, prow, col);
            if (code > 2u) continue;                                 // no call: nothing anywhere
            double q[KT], p, pbar, u, v;
#pragma unroll
            for (int k = 0; k < KT; ++k) q[k] = Q[c * KT + k];
            adm_mix<KT>(q, f, fb, p, pbar);
            adm_ratios(code, p, pbar, u, v);
            ll += adm_loglik(code, p, pbar);
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                a[k] = fma(u, q[k], a[k]);
                b[k] = fma(v, q[k], b[k]);
            }
        }
        const double sa = adm_wave_sum<KT, WAVE / 2>(a, lane), sb = adm_wave_sum<KT, WAVE / 2>(b, lane);
#pragma unroll
        for (int o = WAVE / 2; o >= 1; o >>= 1) ll += pca_shfl_xor(ll, o);
        ll_wave += ll;
        const int comp = lane >> sh;
        if (update_f && (lane & ((1 << sh) - 1)) == 0 && comp < K) {
            const double fk = F[s * KT + comp];
            const double x = fk * sa, y = (1.0 - fk) * sb, den = x + y;
            double fn = fk;
            if (den != 0.0) {
                fn = x / den;
                fn = fn < SNPM_ADMIX_EPS ? SNPM_ADMIX_EPS : fn > 1.0 - SNPM_ADMIX_EPS ? 1.0 - SNPM_ADMIX_EPS : fn;
            }
            F_new[s * KT + comp] = fn;
        }
    }
    if (lane == 0) s_ll[wave] = ll_wave;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = s_ll[0];
        for (int w = 1; w < waves; ++w) sum += s_ll[w];
        ll_blk[blockIdx.x] = sum;
    }
}

// grid (ceil(ncols / ADM_COLS_THREADS), adm_splits(n_rows, ncols)); split_rows = adm_split_rows(n_rows, ncols).  Rows and columns as
// for k_adm_rows.  part [gridDim.y][ncols][KT]: every entry is written.
template <int KT>
__global__ void __launch_bounds__(ADM_COLS_THREADS)
k_adm_cols(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, const int64_t *__restrict__ row_idx, int64_t first, int64_t n_rows,
           int64_t split_rows, const int32_t *__restrict__ cols, int64_t ncols, const double *__restrict__ Q, const double *__restrict__ F,
           double *__restrict__ part)
{
    __shared__ double s_f[ADM_CHUNK_ROWS * KT];
    __shared__ int64_t s_row[ADM_CHUNK_ROWS];
    const int64_t c = (int64_t)blockIdx.x * ADM_COLS_THREADS + threadIdx.x;
    const bool active = c < ncols;
    const int64_t col = active ? (cols ? (int64_t)cols[c] : c) : 0;
    double q[KT], acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        q[k] = active ? Q[c * KT + k] : 0.0;
        acc[k] = 0.0;
    }
    const int64_t r0 = (int64_t)blockIdx.y * split_rows, r1 = r0 + split_rows < n_rows ? r0 + split_rows : n_rows;
    for (int64_t base = r0; base < r1; base += ADM_CHUNK_ROWS) {     // (block-uniform)
        const int n = (int)(r1 - base < ADM_CHUNK_ROWS ? r1 - base : ADM_CHUNK_ROWS);
        __syncthreads();                                             // the previous chunk has been read
        for (int i = threadIdx.x; i < n * KT; i += ADM_COLS_THREADS) s_f[i] = F[base * KT + i];
        if ((int)threadIdx.x < n) s_row[threadIdx.x] = row_idx ? row_idx[first + base + threadIdx.x] : first + base + threadIdx.x;
        __syncthreads();
        if (!active) continue;
        for (int j = 0; j < n; ++j) {
            const uint32_t code = kin_code(db, pitch, desc, s_row[j], col);
            if (code > 2u) continue;
            double f[KT], fb[KT], p, pbar, u, v;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                f[k] = s_f[j * KT + k];
                fb[k] = 1.0 - f[k];
            }
            adm_mix<KT>(q, f, fb, p, pbar);
            adm_ratios(code, p, pbar, u, v);
#pragma unroll
            for (int k = 0; k < KT; ++k) acc[k] = fma(v, fb[k], fma(u, f[k], acc[k]));
        }
    }
    if (active) {
        double *out = part + ((int64_t)blockIdx.y * ncols + c) * KT;
#pragma unroll
        for (int k = 0; k < KT; ++k) out[k] = acc[k];
    }
}

// grid (column blocks + 1), column blocks = adm_fold_col_blocks(ncols, KT) with SNPM_ADMIX_UPDATE_Q, else 0: a thread per (listed
// column, component), the KT threads of a column side by side, so the reads of the partials are contiguous.  Q and Q_new [ncols][KT]:
// every entry of Q_new is written.  ll_a [n_ll] holds ll_blk of k_adm_rows and ll_b [ceil(n_ll / ADM_TREE_RADIX)] is scratch: both are
// overwritten; *loglik_t receives the sum.  (ll_a / ll_b carry no __restrict__: the levels of the tree swap them.)
template <int KT>
__global__ void __launch_bounds__(ADM_FOLD_THREADS)
k_adm_fold(const double *__restrict__ part, int64_t splits, int64_t ncols, const double *__restrict__ Q, double *__restrict__ Q_new,
           double *ll_a, double *ll_b, int64_t n_ll, double *__restrict__ loglik_t)
{
    if (blockIdx.x + 1 < gridDim.x) {                               // (block-uniform)
        __shared__ double s_w[ADM_FOLD_THREADS];
        const int k = threadIdx.x % KT, lc = threadIdx.x / KT;
        const int64_t c = (int64_t)blockIdx.x * (ADM_FOLD_THREADS / KT) + lc;
        double q = 0.0, w = 0.0;
        if (c < ncols) {
            double cs = part[c * KT + k];
            for (int64_t s = 1; s < splits; ++s) cs += part[(s * ncols + c) * KT + k];
            q = Q[c * KT + k];
            w = q * cs;
        }
        s_w[threadIdx.x] = w;
        __syncthreads();
        if (c < ncols) {                                             // the KT threads of a column add the same values in the same order
            double sum = 0.0;
            for (int j = 0; j < KT; ++j) sum += s_w[lc * KT + j];
            Q_new[c * KT + k] = sum != 0.0 ? w / sum : q;
        }
        return;
    }
    double *src = ll_a, *dst = ll_b;
    for (int64_t n = n_ll; n > 1; n = (n + ADM_TREE_RADIX - 1) / ADM_TREE_RADIX) {      // (block-uniform)
        const int64_t m = (n + ADM_TREE_RADIX - 1) / ADM_TREE_RADIX;
        for (int64_t j = threadIdx.x; j < m; j += ADM_FOLD_THREADS) {
            double sum = src[ADM_TREE_RADIX * j];
            for (int i = 1; i < ADM_TREE_RADIX; ++i)
                if (ADM_TREE_RADIX * j + i < n) sum += src[ADM_TREE_RADIX * j + i];
            dst[j] = sum;
        }
        __syncthreads();                                             // (a barrier of the block orders its global writes as well)
        double *t = src;
        src = dst;
        dst = t;
    }
    if (threadIdx.x == 0) *loglik_t = src[0];
}

}  // namespace snpm
