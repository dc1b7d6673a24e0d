// snpm_k_pca.hpp -- pca: the weighted Gram matrix of the accession columns over panel rows (the genotype relationship matrix before its division by the row count) and the row-streaming product for the SNP loadings.  The package's own command: the reference has no counterpart (its calc_kinship_mat is the count form, snpm_k_kin.hpp).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp and kin_code of
// snpm_k_kin.hpp only (the planes come from k_win_planes of snpm_k_win.hpp), so that tests/pca_host_driver.cpp can compile this very
// text for the host (tests/host_kernel/).
#pragma once

#ifndef SNPM_PCA_MAX_ACCESSIONS
#define SNPM_PCA_MAX_ACCESSIONS 11552       // (include/snpmatch_hip.h carries the same figures for callers)
#endif
#ifndef SNPM_PCA_MAX_COMPONENTS
#define SNPM_PCA_MAX_COMPONENTS 32
#endif

namespace snpm {
// ------------------------------------------------------------------------------------------------
// A CLASS TABLE tab [n_rows][4] of fp64 gives selected row s a value per canonical code (kin_code: 0 ref, 1 alt, 2 het, 3 an int8
// panel's "other"); a missing call has value 0.  With t(s, i) = tab[s][code(s, i)], or 0 where missing:
//   gram[i][j] = sum over selected rows s of t(s, i) * t(s, j)            (k_pca_gram + k_pca_fold, behind k_win_planes)
//   load[s][c] = sum over listed columns i of t(s, i) * vec[i][c]         (k_pca_load, from the panel rows directly)
// Every other pair scan of the package is a popcount of bit-planes, where every row weighs the same; here every row has its own
// four weights, so the planes are DECODED to fp64 values and the pair scan is a rank-R update in fp64.  All arithmetic is fp64
// FMA; there is no floating-point atomic: every output cell has one owner and one order of summation, fixed by the arguments and
// the workspace budget, so the same call returns the same bits.
//
// k_pca_gram, per SLAB of rows (the host cuts the row axis, pca_slab_steps), behind k_win_planes AS IT STANDS (planes
// [4][cols_pad][W]: P0, P1, P2, I; padding rows and columns are zero bits, so they decode to 0):
//   grid (tile pair ta <= tb, split).  A block owns the PCA_TILE x PCA_TILE cells of its tile pair for the plane steps of its
//   split (the steps of the slab are dealt to the splits in contiguous runs: pca_gram_splits blocks per tile pair keep every CU
//   busy at widths where the tile pairs alone would not).  It walks its rows PCA_KROWS at a time: every thread decodes eight
//   (row, accession) values per side from the four plane bits and the row's table entries -- four selects, no branch -- into LDS
//   as fp64, a[k][accession] and b[k][accession]; then a 4 x 4 register tile of cells per lane takes one FMA per cell and row
//   from 4 + 4 LDS reads of 8 bytes: the lanes of a half wave read 16 consecutive doubles of b (every bank pair once), the four
//   values of a are one address per quarter wave (broadcast).  The cell's sum runs over its rows in row order.  The block STORES
//   its 64 x 64 partial sums into part[split][pair][64][64]: no cell of part has two writers.
// k_pca_fold: a thread per cell (i, j) of the FULL matrix adds the partials of its tile pair, split 0 first, then adds that sum to
//   gram[i][j] (zeroed before the first slab: the matrix accumulates on the device in slab order).  (i, j) and (j, i) read the
//   same partials in the same order, so the matrix is symmetric bit for bit.
// With small-integer tables every partial sum is an exact integer and so is the result, whatever the order.
//
// fp64 v_mfma was not used: it runs at the rate of the fp64 vector FMA (head of snpm_k_shared.hpp), so it would save LDS reads and
// registers, not time on the FMA pipe, and the register tile keeps the text runnable on the host as it stands.
//
// k_pca_load: a wave per selected row, the scheme of k_site_counts without its indicator words: lane l takes listed columns l,
//   l + 64, ..., reads the call with kin_code, selects its value and adds value * vec[i][c] into one accumulator per component
//   (SNPM_PCA_MAX_COMPONENTS of them, statically indexed; components go in groups of PCA_LOAD_GROUP, the host pads the rows of vec
//   with zeros to whole groups, groups at or beyond k are skipped by a wave-uniform test); a halving exchange -- 32 exchanges in
//   six steps for all components together -- sums the lanes and leaves component c in lane 2 c, which stores it.  It reads the panel rows directly because a row
//   is read once whichever way, and planes would add a write and a read of 4 bits per call and the transposed access (a row's
//   calls sit in ncols different plane rows) for nothing.
constexpr int PCA_TILE = 64;                // accessions per tile side of k_pca_gram
constexpr int PCA_THREADS = 256;
constexpr int PCA_KROWS = 32;               // rows decoded into LDS at a time: half a plane word
constexpr int PCA_STEP_WORDS = 16;          // 64-bit words (= 1024 rows) per plane step (WN_STEP_WORDS); W is a multiple of it
constexpr int PCA_PL_COLS = 64;             // accessions per tile of k_win_planes: cols_pad is a multiple of it
constexpr int PCA_MAX_SPLITS = 32;
constexpr int PCA_BLOCKS_WANTED = 512;      // two blocks per CU of a 256-CU device
constexpr int64_t PCA_STEP_ROWS = (int64_t)PCA_STEP_WORDS * 64;
constexpr int PCA_LOAD_THREADS = 256;
constexpr int PCA_LOAD_GROUP = 8;           // components per group of k_pca_load: vec rows are padded to whole groups
static_assert(SNPM_PCA_MAX_COMPONENTS * 2 == WAVE, "the halving exchange of k_pca_load ends with one component per lane pair");
static_assert(SNPM_PCA_MAX_COMPONENTS % PCA_LOAD_GROUP == 0, "whole groups of components");
static_assert(PCA_TILE == PCA_PL_COLS, "a count tile is a plane tile: every accession of a tile has a plane row");
static_assert(PCA_TILE * PCA_TILE == 16 * PCA_THREADS, "a 4 x 4 register tile of cells per lane");
static_assert(PCA_KROWS * PCA_TILE == 8 * PCA_THREADS && 64 % PCA_KROWS == 0, "eight values per thread, side and pass; whole passes per word");

// bytes of one plane step of a slab on the device: the four planes and the table rows of its 1024 rows
__host__ __device__ __forceinline__ int64_t pca_step_bytes(int64_t cols_pad) { return 4 * cols_pad * PCA_STEP_WORDS * 8 + PCA_STEP_ROWS * 32; }

// The host's slab plan of snpm_panel_gram: plane steps of one slab -- as many as fit ws_bytes, at least one whatever the budget (the
// minimum that always fits one step), no more than the rows need.
__host__ __device__ __forceinline__ int64_t pca_slab_steps(size_t ws_bytes, int64_t cols_pad, int64_t n_rows)
{
    const int64_t need = (n_rows + PCA_STEP_ROWS - 1) / PCA_STEP_ROWS;
    int64_t steps = (int64_t)(ws_bytes / (size_t)pca_step_bytes(cols_pad));
    if (steps < 1) steps = 1;
    return steps < need ? steps : need;
}

// blocks per tile pair: a function of the width alone, so the order of summation is fixed by the arguments
__host__ __device__ __forceinline__ int pca_gram_splits(int64_t n_pairs)
{
    const int64_t s = (PCA_BLOCKS_WANTED + n_pairs - 1) / n_pairs;
    return (int)(s < 1 ? 1 : s > PCA_MAX_SPLITS ? PCA_MAX_SPLITS : s);
}

// the slab plan of snpm_panel_loadings: rows whose table (32 B), result (8 k B) and list entry (8 B) fit ws_bytes; at least 64
__host__ __device__ __forceinline__ int64_t pca_load_slab_rows(size_t ws_bytes, int k, int64_t n_rows)
{
    const int64_t fit = (int64_t)(ws_bytes / (size_t)(40 + 8 * k)), rows = fit < 64 ? 64 : fit;
    return rows < n_rows ? rows : n_rows;
}

// doubles per row of the padded vec of k_pca_load
__host__ __device__ __forceinline__ int pca_load_pitch(int k) { return (k + PCA_LOAD_GROUP - 1) / PCA_LOAD_GROUP * PCA_LOAD_GROUP; }

// the value of a call from its four plane bits (P0, P1, P2 exclusive and inside I) and the row's table entries
__device__ __forceinline__ double pca_value(bool b0, bool b1, bool b2, bool bi, double t0, double t1, double t2, double t3)
{
    double v = bi ? t3 : 0.0;
    v = b2 ? t2 : v;
    v = b1 ? t1 : v;
    return b0 ? t0 : v;
}

// grid (tile pairs, splits): blockIdx.x counts the pairs (ta, tb) with ta <= tb row by row.  planes [4][cols_pad][W] of this slab,
// W a multiple of PCA_STEP_WORDS; tab: the table rows of this slab, n_valid of them (row k of the slab is bit k of a plane row);
// part [gridDim.y][gridDim.x][PCA_TILE][PCA_TILE]: every cell is written.
__global__ void __launch_bounds__(PCA_THREADS)
k_pca_gram(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, const double *__restrict__ tab, int64_t n_valid,
           int n_tiles, double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) double s_a[PCA_KROWS * PCA_TILE];         // [row][accession]
    __shared__ __attribute__((aligned(16))) double s_b[PCA_KROWS * PCA_TILE];
    int ta = 0, rest = blockIdx.x;                                  // (block-uniform) row ta of the triangle holds n_tiles - ta pairs
    while (rest >= n_tiles - ta) { rest -= n_tiles - ta; ++ta; }
    const int tb = ta + rest;
    const bool diag = ta == tb;
    const double *sb = diag ? s_a : s_b;
    const int64_t n_steps = W / PCA_STEP_WORDS, per = (n_steps + gridDim.y - 1) / gridDim.y;
    const int64_t st0 = (int64_t)blockIdx.y * per, st1 = st0 + per < n_steps ? st0 + per : n_steps;
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;          // cells {ti + 16 x} of tile ta x {tj + 16 y} of tile tb
    const int sa = threadIdx.x & (PCA_TILE - 1), sg = threadIdx.x >> 6;     // staging: accession sa of the tile, rows 8 sg .. 8 sg + 7 of the pass
    const int64_t plane = cols_pad * W;
    const unsigned long long *pa = planes + ((int64_t)ta * PCA_TILE + sa) * W, *pb = planes + ((int64_t)tb * PCA_TILE + sa) * W;
    double acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;
    for (int64_t w = st0 * PCA_STEP_WORDS; w < st1 * PCA_STEP_WORDS; ++w) {
        if (w * 64 >= n_valid) break;                                // (block-uniform) padding rows only from here on: zero bits, value 0
        const unsigned long long a0 = pa[w], a1 = pa[plane + w], a2 = pa[2 * plane + w], ai = pa[3 * plane + w];
        unsigned long long b0 = 0ull, b1 = 0ull, b2 = 0ull, bi = 0ull;
        if (!diag) { b0 = pb[w]; b1 = pb[plane + w]; b2 = pb[2 * plane + w]; bi = pb[3 * plane + w]; }
        for (int h = 0; h < 64 / PCA_KROWS; ++h) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int kk = 8 * sg + q, bit = h * PCA_KROWS + kk;
                const int64_t r = w * 64 + bit;
                double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
                if (r < n_valid) {                                   // no table row at or past the slab's end is read
                    const double *t = tab + 4 * r;
                    t0 = t[0]; t1 = t[1]; t2 = t[2]; t3 = t[3];
                }
                s_a[kk * PCA_TILE + sa] = pca_value((a0 >> bit) & 1ull, (a1 >> bit) & 1ull, (a2 >> bit) & 1ull, (ai >> bit) & 1ull, t0, t1, t2, t3);
                if (!diag)
                    s_b[kk * PCA_TILE + sa] = pca_value((b0 >> bit) & 1ull, (b1 >> bit) & 1ull, (b2 >> bit) & 1ull, (bi >> bit) & 1ull, t0, t1, t2, t3);
            }
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < PCA_KROWS; ++k) {
                double av[4], bv[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    av[x] = s_a[k * PCA_TILE + ti + 16 * x];
                    bv[x] = sb[k * PCA_TILE + tj + 16 * x];
                }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[x][y] = fma(av[x], bv[y], acc[x][y]);
            }
            __syncthreads();
        }
    }
    double *out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (PCA_TILE * PCA_TILE);
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) out[(ti + 16 * x) * PCA_TILE + tj + 16 * y] = acc[x][y];
}

// grid (ceil(ncols^2 / PCA_THREADS)): gram[i][j] += the partials of cell (i, j), split 0 first.  n_pairs = n_tiles (n_tiles + 1) / 2.
__global__ void __launch_bounds__(PCA_THREADS)
k_pca_fold(const double *__restrict__ part, int n_tiles, int n_pairs, int splits, int64_t ncols, double *__restrict__ gram)
{
    const int64_t cell = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (cell >= ncols * ncols) return;
    const int64_t i = cell / ncols, j = cell - i * ncols;
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    const int64_t ta = lo / PCA_TILE, tb = hi / PCA_TILE;
    const int64_t pair = ta * n_tiles - ta * (ta - 1) / 2 + (tb - ta);
    const double *p = part + pair * (PCA_TILE * PCA_TILE) + (lo - ta * PCA_TILE) * PCA_TILE + (hi - tb * PCA_TILE);
    double sum = p[0];
    for (int s = 1; s < splits; ++s) sum += p[(int64_t)s * n_pairs * (PCA_TILE * PCA_TILE)];
    gram[cell] += sum;
}

// the value of another lane, a double as two 32-bit exchanges
__device__ __forceinline__ double pca_shfl_xor(double v, int lane_mask)
{
    unsigned long long u;
    memcpy(&u, &v, 8);
    const uint32_t lo = __shfl_xor((uint32_t)u, lane_mask), hi = __shfl_xor((uint32_t)(u >> 32), lane_mask);
    u = (unsigned long long)lo | ((unsigned long long)hi << 32);
    memcpy(&v, &u, 8);
    return v;
}

// grid (blocks), any number: the waves stride the rows of the slab.  Row k of the slab (0 <= k < n_valid) is panel row
// row_idx[first + k], or first + k when row_idx is null; column a of the call (0 <= a < ncols) is panel column cols[a], or a when cols
// is null.  tab [n_valid][4] and load [n_valid][k]: the slab's; 1 <= k <= SNPM_PCA_MAX_COMPONENTS; vec [ncols][kp], kp = k rounded up
// to PCA_LOAD_GROUP, the entries at and beyond k zero (the host pads): components go in whole groups, the test per group is wave-uniform.
__global__ void __launch_bounds__(PCA_LOAD_THREADS)
k_pca_load(const int8_t *__restrict__ db, int64_t pitch, int64_t desc, const int64_t *__restrict__ row_idx, int64_t first, int64_t n_valid,
           const int32_t *__restrict__ cols, int64_t ncols, const double *__restrict__ tab, const double *__restrict__ vec, int k,
           double *__restrict__ load)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    const int kp = pca_load_pitch(k);
    constexpr int waves = PCA_LOAD_THREADS / WAVE, groups = SNPM_PCA_MAX_COMPONENTS / PCA_LOAD_GROUP;
    for (int64_t s = (int64_t)blockIdx.x * waves + wave; s < n_valid; s += (int64_t)gridDim.x * waves) {     // (wave-uniform)
        const int64_t prow = row_idx ? row_idx[first + s] : first + s;
        const double t0 = tab[4 * s], t1 = tab[4 * s + 1], t2 = tab[4 * s + 2], t3 = tab[4 * s + 3];
        double acc[SNPM_PCA_MAX_COMPONENTS];
#pragma unroll
        for (int c = 0; c < SNPM_PCA_MAX_COMPONENTS; ++c) acc[c] = 0.0;
        for (int64_t a = lane; a < ncols; a += WAVE) {
            const int64_t col = cols ? (int64_t)cols[a] : a;
            const uint32_t v = kin_code(db, pitch, desc, prow, col);
            const double t = pca_value(v == 0u, v == 1u, v == 2u, v != 0xFFu, t0, t1, t2, t3);
            const double *vr = vec + a * kp;
#pragma unroll
            for (int g = 0; g < groups; ++g) {
                if (g * PCA_LOAD_GROUP >= kp) break;
#pragma unroll
                for (int c = g * PCA_LOAD_GROUP; c < (g + 1) * PCA_LOAD_GROUP; ++c) acc[c] = fma(t, vr[c], acc[c]);
            }
        }
        // the lanes' sums: every exchange halves the components a lane holds -- at distance o the lanes with (lane & o) set keep the
        // upper half of their components and send the lower, the others the other way round -- so 16 + 8 + 4 + 2 + 1 exchanges
        // leave component (lane >> 1) in every lane, summed over the 32 lanes that share its upper bits, and one more sums the pair
        double r[SNPM_PCA_MAX_COMPONENTS];
#pragma unroll
        for (int c = 0; c < SNPM_PCA_MAX_COMPONENTS; ++c) r[c] = acc[c];
#pragma unroll
        for (int n = SNPM_PCA_MAX_COMPONENTS / 2, o = WAVE / 2; n >= 1; n >>= 1, o >>= 1) {
            const bool up = (lane & o) != 0;
#pragma unroll
            for (int c = 0; c < n; ++c) {
                const double keep = up ? r[c + n] : r[c], send = up ? r[c] : r[c + n];
                r[c] = keep + pca_shfl_xor(send, o);
            }
        }
        const double sum = r[0] + pca_shfl_xor(r[0], 1);
        if ((lane & 1) == 0 && (lane >> 1) < k) load[s * k + (lane >> 1)] = sum;
    }
}

}  // namespace snpm
