// snpm_k_gcross.hpp -- genotype_cross: per (genome window, F2 sample) parental call (core/genotype_cross.py:21-49, :184-195 of the reference).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one: it uses likeli_one of snpm_k_post.hpp).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Input: the call codes of every sample at the matched segregating markers, marker-major [n, pitch] with the samples contiguous
// (the place the accessions have in the panel), the two parents' calls per marker and the window bounds.
//   code byte: bits 0-2 class (0 '0s0', 1 '1s1', 2 '0s1' / '1s0', 3 '.s.', 4 anything else with a separator), bit 3 the separator is '|'
//   value of an element: {0, 1, 2, -1, 0}[class] when its separator is the one of the (window, sample)'s FIRST row, else 0
//   (parseGT takes the separator from the first genotype it is given and compares whole strings, core/parsers.py:12-35)
//   m1 = #(value == p1), mh = #(value == 2), m2 = #(value == p2), tot = rows of the window
//
// Decomposition: grid (window, tile of 256 samples), 256 threads.  A lane owns four adjacent samples (one aligned 4-byte load per
// row: `pitch` is a multiple of 4 and the buffer is the library's own, so the load of the last lane stays inside the row); the
// four waves take rows start + wave, start + wave + 4, ... of the window, so the row number, p1[r], p2[r] and the window bounds
// are wave-uniform (scalar loads).  The int32 counts of the four waves meet in LDS; then thread (wave w, lane l) owns sample
// 4 l + w of the tile, adds the four partial counts and decides.  A window of 700 rows is 175 loads per wave, a window of 0 rows
// reads nothing (not even a first row: there is none), a tile with one sample has one useful lane -- correct, not fast.
constexpr int GC_THREADS = 256;
constexpr int GC_SAMPLES_PER_LANE = 4;
constexpr int GC_TILE = WAVE * GC_SAMPLES_PER_LANE;

// getWindowGenotype (core/genotype_cross.py:21-49): -1 = 'NA'
__device__ __forceinline__ int gc_decide(int m1, int mh, int m2, int tot, double lr_thres, int n_marker_thres)
{
    if (tot < n_marker_thres) return -1;
    if (m1 == 0 && mh == 0 && m2 == 0) return -1;
    int bad = 0;
    const double n = (double)tot;
    const double l0 = likeli_one((double)m1, n, &bad);
    const double l1 = likeli_one((double)mh, n, &bad);
    const double l2 = likeli_one((double)m2, n, &bad);
    // np.nanmin / np.nanargmin: the first index of the smallest value that is not NaN (one exists: some count is > 0)
    double mn = __builtin_inf();
    int high = -1;
    if (l0 == l0 && l0 < mn) { mn = l0; high = 0; }
    if (l1 == l1 && l1 < mn) { mn = l1; high = 1; }
    if (l2 == l2 && l2 < mn) { mn = l2; high = 2; }
    // get_fraction(x, top): NaN when top <= 0 (core/snpmatch.py:25-28)
    const bool ok = mn > 0.0;
    const double nan = __builtin_nan("");
    const double r0 = ok ? l0 / mn : nan, r1 = ok ? l1 / mn : nan, r2 = ok ? l2 / mn : nan;
    if ((int)(r0 == 1.0) + (int)(r1 == 1.0) + (int)(r2 == 1.0) > 1) return 1;
    // np.nanmin over the ratios with ratio - 1 != 0 (NaN - 1 != 0 holds: NaNs are in the set and nanmin skips them); all NaN -> lr_thres
    double next = __builtin_inf();
    bool any = false;
    if (r0 == r0 && r0 - 1.0 != 0.0) { next = r0 < next ? r0 : next; any = true; }
    if (r1 == r1 && r1 - 1.0 != 0.0) { next = r1 < next ? r1 : next; any = true; }
    if (r2 == r2 && r2 - 1.0 != 0.0) { next = r2 < next ? r2 : next; any = true; }
    if (!any) next = lr_thres;
    int g = -1;
    if (high == 0 && next >= lr_thres) g = 0;
    else if (high == 2 && next >= lr_thres) g = 2;
    if (high == 1) g = 1;
    return g;
}

__global__ void __launch_bounds__(GC_THREADS)
k_gcross(const uint8_t *__restrict__ codes, int64_t pitch, int n_samples, const int8_t *__restrict__ p1, const int8_t *__restrict__ p2,
         const int64_t *__restrict__ win_off, double lr_thres, int n_marker_thres, int8_t *__restrict__ geno, int32_t *__restrict__ counts)
{
    __shared__ int s_cnt[4 * GC_SAMPLES_PER_LANE * 3 * WAVE];      // [wave][sample of the lane][m1, mh, m2][lane]
    const int w = blockIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t start = win_off[w], end = win_off[w + 1];
    const int s0 = blockIdx.y * GC_TILE + lane * GC_SAMPLES_PER_LANE;          // first of this lane's four samples
    const bool active = s0 < n_samples;                                         // (s0 + 3 < pitch then: pitch >= n_samples rounded up to 4)
    int c[GC_SAMPLES_PER_LANE][3];
#pragma unroll
    for (int j = 0; j < GC_SAMPLES_PER_LANE; ++j) c[j][0] = c[j][1] = c[j][2] = 0;
    if (active && start < end) {
        const uint32_t first = *(const uint32_t *)(codes + start * pitch + s0);
        const uint32_t gov = (first >> 3) & 0x01010101u;                        // governing separator of each of the four samples
#pragma unroll 4
        for (int64_t r = start + wave; r < end; r += 4) {
            const uint32_t v4 = *(const uint32_t *)(codes + r * pitch + s0);
            const int a = p1[r], b = p2[r];
            const uint32_t same = ~((v4 >> 3) ^ gov);                           // bit 0 of each byte: the element's separator is the governing one
#pragma unroll
            for (int j = 0; j < GC_SAMPLES_PER_LANE; ++j) {
                const int cls = (int)((v4 >> (8 * j)) & 7u);
                const bool mine = (same >> (8 * j)) & 1u;
                // {0, 1, 2, -1, 0}[cls] under the governing separator, 0 under the other one
                const int val = mine ? (cls == 3 ? -1 : (cls <= 2 ? cls : 0)) : 0;
                c[j][0] += (val == a);
                c[j][1] += (val == 2);
                c[j][2] += (val == b);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < GC_SAMPLES_PER_LANE; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) s_cnt[((wave * GC_SAMPLES_PER_LANE + j) * 3 + k) * WAVE + lane] = c[j][k];
    __syncthreads();
    const int s = blockIdx.y * GC_TILE + lane * GC_SAMPLES_PER_LANE + wave;     // the sample this thread decides
    if (s >= n_samples) return;
    int m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int t = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) t += s_cnt[((v * GC_SAMPLES_PER_LANE + wave) * 3 + k) * WAVE + lane];
        m[k] = t;
    }
    const int64_t o = (int64_t)w * n_samples + s;
    geno[o] = (int8_t)gc_decide(m[0], m[1], m[2], (int)(end - start), lr_thres, n_marker_thres);
    if (counts) {
        counts[o * 3 + 0] = m[0];
        counts[o * 3 + 1] = m[1];
        counts[o * 3 + 2] = m[2];
    }
}

}  // namespace snpm
