// snpm_k_ghmm.hpp -- genotype_cross_hmm: 3-state Viterbi (AA / AB / BB) of every (chain, F2 sample) (core/infer.py:17-58, :173-310 of the reference).
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Input: the call codes (snpm_k_gcross.hpp) and the depth ranks of every sample at the matched segregating markers, marker-major
// [n, pitch] with the samples contiguous, the ordered parental pair of every marker, the marker range of every chain (one chain =
// one chromosome) and three tables of logarithms the HOST computed with numpy: no logarithm runs here.
//   observation of an element: {0, 2, 1, 3, 0}[class] when its separator is the one of the (chain, sample)'s FIRST row, else 0
//   (parseGT's governing separator, then snp_to_observations: 0 -> 0, 2 -> 1, 1 -> 2, -1 -> 3)
//   table entry of (marker r, sample s): t = ((pair[r] * n_depth + depth_rank[r][s]) * 4 + observation) * 3, three doubles (per state)
//   omega[start] = logI[t .. t + 2];  omega[r][j] = max_i ((omega[r - 1][i] + logT[i][j]) + logE[t + j]), the FIRST maximum over
//   i = 0, 1, 2 (np.argmax / np.max: a strict > against a running best that starts at i = 0, also when all three are -inf)
//
// Decomposition: grid (chain, tile of 64 samples), one wave per block, one lane = one chain of one sample from its first marker
// to its last and back.  The marker index, pair[r] and the chain bounds are wave-uniform; the code, depth-rank and backpointer
// accesses of a step are 64 adjacent elements.  The symbol and table loads of a step do not depend on omega: they are issued
// GH_UNROLL steps ahead (the block after the one being computed), so the dependent chain of a step is two additions and two
// compares per target state.  The three 2-bit backpointers of a step share one byte of the workspace `bp` [n, pitch]; the lane
// that wrote them walks them back after its last marker and writes state [n, pitch].  Rows past the chain's end are never
// addressed: a prefetch beyond the end re-reads the chain's last row (clamped, wave-uniform) and its values are not used.
// Lanes at or beyond n_samples leave at once (no barrier follows).  All row * pitch products are int64.
constexpr int GH_UNROLL = 8;

struct GhStep {
    double e0, e1, e2;
};

__device__ __forceinline__ int gh_observation(uint32_t code, uint32_t gov)
{
    const uint32_t cls = code & 7u;
    const bool mine = ((code >> 3) & 1u) == gov;
    // class 0 '0s0' -> 0, 1 '1s1' -> 2, 2 '0s1' -> 1, 3 '.s.' -> 3, 4 (anything else) -> 0; the other separator reads as '0s0'
    const int obs = cls == 1u ? 2 : (cls == 2u ? 1 : (cls == 3u ? 3 : 0));
    return mine ? obs : 0;
}

__global__ void __launch_bounds__(WAVE)
k_ghmm(const uint8_t *__restrict__ codes, const uint16_t *__restrict__ depth, int64_t pitch, int n_samples,
       const uint8_t *__restrict__ pair, const int64_t *__restrict__ chain_off, const double *__restrict__ logT,
       const double *__restrict__ logI, const double *__restrict__ logE, int n_depth, uint8_t *bp, int8_t *__restrict__ state,
       double *__restrict__ omega)
{
    const int chain = blockIdx.x;
    const int s = blockIdx.y * WAVE + (int)threadIdx.x;
    const int64_t start = chain_off[chain], end = chain_off[chain + 1];
    if (s >= n_samples || start >= end) return;
    const uint32_t gov = ((uint32_t)codes[start * pitch + s] >> 3) & 1u;
    const double *T = logT + (int64_t)chain * 9;
    const double t00 = T[0], t01 = T[1], t02 = T[2], t10 = T[3], t11 = T[4], t12 = T[5], t20 = T[6], t21 = T[7], t22 = T[8];

    // table offset of (row r, this sample)
    auto entry = [&](int64_t r) -> int64_t {
        const int64_t at = r * pitch + s;
        const int obs = gh_observation(codes[at], gov);
        return (((int64_t)pair[r] * n_depth + (int64_t)depth[at]) * 4 + obs) * 3;
    };
    auto fetch = [&](int64_t r) -> GhStep {
        const int64_t rr = r < end ? r : end - 1;          // past the end: the last row again, never another chain's or none
        const double *e = logE + entry(rr);
        return GhStep{e[0], e[1], e[2]};
    };

    double om0, om1, om2;
    {
        const double *i0 = logI + entry(start);
        om0 = i0[0];
        om1 = i0[1];
        om2 = i0[2];
    }
    if (omega) {
        double *o = omega + (start * (int64_t)n_samples + s) * 3;
        o[0] = om0;
        o[1] = om1;
        o[2] = om2;
    }
    GhStep cur[GH_UNROLL], nxt[GH_UNROLL];
#pragma unroll
    for (int u = 0; u < GH_UNROLL; ++u) cur[u] = fetch(start + 1 + u);
    for (int64_t r0 = start + 1; r0 < end; r0 += GH_UNROLL) {
#pragma unroll
        for (int u = 0; u < GH_UNROLL; ++u) nxt[u] = fetch(r0 + GH_UNROLL + u);
#pragma unroll
        for (int u = 0; u < GH_UNROLL; ++u) {
            const int64_t r = r0 + u;
            if (r < end) {                                  // wave-uniform
                // target state j: ((omega[i] + logT[i][j]) + logE[j]) for i = 0, 1, 2; first maximum
                double b0 = (om0 + t00) + cur[u].e0;
                double c = (om1 + t10) + cur[u].e0;
                uint32_t k0 = 0;
                if (c > b0) { b0 = c; k0 = 1; }
                c = (om2 + t20) + cur[u].e0;
                if (c > b0) { b0 = c; k0 = 2; }
                double b1 = (om0 + t01) + cur[u].e1;
                c = (om1 + t11) + cur[u].e1;
                uint32_t k1 = 0;
                if (c > b1) { b1 = c; k1 = 1; }
                c = (om2 + t21) + cur[u].e1;
                if (c > b1) { b1 = c; k1 = 2; }
                double b2 = (om0 + t02) + cur[u].e2;
                c = (om1 + t12) + cur[u].e2;
                uint32_t k2 = 0;
                if (c > b2) { b2 = c; k2 = 1; }
                c = (om2 + t22) + cur[u].e2;
                if (c > b2) { b2 = c; k2 = 2; }
                om0 = b0;
                om1 = b1;
                om2 = b2;
                bp[r * pitch + s] = (uint8_t)(k0 | (k1 << 2) | (k2 << 4));
                if (omega) {
                    double *o = omega + (r * (int64_t)n_samples + s) * 3;
                    o[0] = om0;
                    o[1] = om1;
                    o[2] = om2;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GH_UNROLL; ++u) cur[u] = nxt[u];
    }

    // np.argmax of the last omega, then the lane's own backpointers downwards (their addresses do not depend on the path: the
    // bytes of GH_UNROLL rows are loaded together)
    uint32_t k = 0;
    {
        double best = om0;
        if (om1 > best) { best = om1; k = 1; }
        if (om2 > best) { k = 2; }
    }
    state[(end - 1) * pitch + s] = (int8_t)k;
    for (int64_t r0 = end - 1; r0 > start; r0 -= GH_UNROLL) {
        uint32_t b[GH_UNROLL];
#pragma unroll
        for (int u = 0; u < GH_UNROLL; ++u) {
            const int64_t r = r0 - u;
            b[u] = bp[(r > start ? r : start + 1) * pitch + s];       // rows start + 1 .. end - 1 only (end - start >= 2 here)
        }
#pragma unroll
        for (int u = 0; u < GH_UNROLL; ++u) {
            const int64_t r = r0 - u;
            if (r > start) {                                // wave-uniform
                k = (b[u] >> (2 * k)) & 3u;
                state[(r - 1) * pitch + s] = (int8_t)k;
            }
        }
    }
}

}  // namespace snpm
