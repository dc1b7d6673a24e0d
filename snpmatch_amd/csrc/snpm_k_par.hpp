// snpm_k_par.hpp -- parentsearch: EVERY pair of accession columns scored per genome window as the parents of a recombinant sample (an F2, a backcross, a RIL with residual heterozygosity): in each window the sample is taken as parent A, as parent B or as their F1, whichever fits that window best.
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp, k_win_planes of
// snpm_k_win.hpp (its planes) and the constants and f1x_popc of snpm_k_f1x.hpp only, so that tests/par_host_driver.cpp can compile
// this very text for the host (tests/host_kernel/).  The plan functions below are plain host code.
#pragma once
#include <cstdint>
#include <vector>

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Columns a, b (positions in the column list), canonical codes (kin_code), the sample's class per selected row (0 ref, 1 alt, 2 het,
// 0xFF none), windows [win_off[w], win_off[w + 1]) of the selected rows.  Per cell (a, b) and window, over the rows `ni` where the F1
// of a and b is informative (the rule of snpm_k_f1x.hpp) AND the sample has a class:
//   n = |ni|   hA = #rows of ni where a's code is the sample's class   hB = the same for b   hF = #rows where the F1's class is it
// A window with n < min_win_sites adds nothing.  Else, with hom = max(hA, hB):
//   hF > hom:  score += hF, w_het += 1
//   else:      score += hom, and the window counts in w_first[a, b] when hA > hB or (hA == hB and a <= b), in w_first[b, a] otherwise
//   n_tot += n
// Four int32 matrices [ncols][ncols]; score, n_tot, w_het symmetric, w_first not.
//
// Per SLAB of WHOLE windows (par_plan: the planes of a slab fit a workspace budget, at least one window whatever the budget):
//   planes  k_win_planes AS IT STANDS, `first` = the slab's first selected row (any row): bit k of a plane row is selected row
//       slab.r0 + k, so a window may start and end anywhere inside a word.
//   segments  every count above is gated by a class mask, so the host folds the window boundaries into the masks: a SEGMENT is
//       (S0, S1, S2, meta) -- the three class masks of one 64-bit word already ANDed with a window's bit range, the word's place in
//       its LDS step and an "end of window" flag.  A word holding k boundaries gives up to k + 1 segments; a segment with no class
//       bit is dropped, the flag sits on a window's last kept segment (a window without one has n = 0: it adds nothing).
//   k_par_count  the tiling of k_f1x_count -- F1X_TILE x F1X_TILE pairs per block of 256 threads, a 2 x 2 register tile per lane, five
//       planes per side staged per step of F1X_STEP_WORDS words -- over a GROUP of whole consecutive windows (about F1X_CHUNK_WORDS
//       words; a longer window is a group of its own with more steps).  A block stages whole step-aligned runs of words that cover
//       its group and walks the step's segments (block-uniform loads from the stream; a step may hold 16 + 1024 of them), per pair
//         e0, e1, u, ni, het as in k_f1x_count        S = S0 | S1 | S2
//         mA = (P0a & S0) | (P1a & S1) | (P2a & S2)   mB likewise                    (per side, shared by the lane's two pairs)
//         n += popc(ni & S)   hA += popc(ni & mA)   hB += popc(ni & mB)   hF += popc((e0 & S0) | (e1 & S1) | (het & S2))
//       At a segment that ends a window (block-uniform branch) the lane takes the maximum, adds into its five totals (score, n_tot,
//       w_first for a, w_first for b, w_het) and clears the four counters.  Totals go into the zeroed matrices with int32 atomicAdd;
//       a block off the diagonal writes score / n_tot / w_het to both cells, its w_first for a to [a, b] and for b to [b, a]; a
//       diagonal block holds both (a, b) and (b, a) as pairs of its own and writes only its own cell.
constexpr int PAR_THREADS = F1X_THREADS;
constexpr int PAR_MIN_BLOCKS = 3;           // blocks per CU the register budget is set for (__launch_bounds__): the three the LDS allows; the kernel takes 104 VGPRs of the 168 that leaves
constexpr int PAR_SEG_WORDS = 4;            // 64-bit words of a segment: S0, S1, S2, meta
constexpr unsigned long long PAR_SEG_END = 16ull;      // meta: bits 0..3 the word inside its step, bit 4 "ends a window"
constexpr int PAR_GROUP_WORDS = 3;          // int64 per group: first word (step-aligned, in the slab's planes), steps, index of its first step in step_off
constexpr int64_t PAR_MAX_GRID_Y = 65535;   // groups per launch
static_assert(F1X_STEP_WORDS == 16, "the word inside a step is four bits of meta");

struct ParSlab {
    int64_t w_lo, w_hi;     // windows [w_lo, w_hi)
    int64_t r0, n_rows;     // selected rows [r0, r0 + n_rows): bits 0 .. n_rows - 1 of the slab's plane rows
    int64_t W;              // words per plane row: whole steps
    int64_t g_lo, g_hi;     // groups [g_lo, g_hi)
};

struct ParPlan {
    std::vector<ParSlab> slabs;                 // slabs without a row are not listed
    std::vector<int64_t> groups;                // [n_groups][PAR_GROUP_WORDS]
    std::vector<int64_t> step_off;              // per step of every group, in group order: its first segment; one closing entry
    std::vector<unsigned long long> segs;       // [n_segs][PAR_SEG_WORDS]
    int64_t max_W = 0, max_rows = 0;            // of the largest slab
};

__host__ __device__ __forceinline__ int64_t par_words(int64_t n_rows) { return (n_rows + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS * F1X_STEP_WORDS; }

// Slabs: whole windows while the planes [4][cols_pad][W] fit ws_bytes, at least one window with rows whatever the budget (compared
// in fp64: no product can overflow).  Empty windows ride with their neighbours.
inline void par_plan_slabs(size_t ws_bytes, int64_t cols_pad, const int64_t *win_off, int64_t n_win, ParPlan &plan)
{
    const double word_bytes = (double)F1X_PLANES * (double)cols_pad * 8.0;
    int64_t w = 0;
    while (w < n_win) {
        ParSlab s;
        s.w_lo = w;
        s.r0 = win_off[w];
        int64_t rows = 0;
        while (w < n_win) {
            const int64_t more = win_off[w + 1] - s.r0;
            if (rows > 0 && more > rows && (double)par_words(more) * word_bytes > (double)ws_bytes) break;
            rows = more;
            ++w;
        }
        s.w_hi = w;
        s.n_rows = rows;
        s.W = par_words(rows);
        s.g_lo = s.g_hi = 0;
        if (rows == 0) continue;
        if (s.W > plan.max_W) plan.max_W = s.W;
        if (rows > plan.max_rows) plan.max_rows = rows;
        plan.slabs.push_back(s);
    }
}

// Groups of a slab: whole consecutive windows while their bit span stays within F1X_CHUNK_WORDS words; a longer window is a group
// of its own.  A group's steps are the step-aligned run of words covering its bits.  Windows without a row join no group.
// The group table gets (first word, steps, 0); par_plan_segments fills the third entry.
inline void par_plan_groups(const int64_t *win_off, ParSlab &s, ParPlan &plan, std::vector<int64_t> &group_win)
{
    const int64_t chunk_rows = (int64_t)F1X_CHUNK_WORDS * 64;
    s.g_lo = (int64_t)plan.groups.size() / PAR_GROUP_WORDS;
    int64_t w = s.w_lo;
    while (w < s.w_hi) {
        if (win_off[w + 1] == win_off[w]) { ++w; continue; }
        const int64_t b0 = win_off[w] - s.r0, first = w;
        int64_t b1 = win_off[w + 1] - s.r0;
        ++w;
        while (w < s.w_hi && win_off[w + 1] - s.r0 - b0 <= chunk_rows) b1 = win_off[++w] - s.r0;
        const int64_t step0 = b0 / F1X_STEP_ROWS, step1 = (b1 - 1) / F1X_STEP_ROWS;
        plan.groups.push_back(step0 * F1X_STEP_WORDS);
        plan.groups.push_back(step1 - step0 + 1);
        plan.groups.push_back(0);
        group_win.push_back(first);
        group_win.push_back(w);
    }
    s.g_hi = (int64_t)plan.groups.size() / PAR_GROUP_WORDS;
}

// Segments of the groups [s.g_lo, s.g_hi) of a slab, whose windows are group_win[2 g], group_win[2 g + 1] (g counted over the plan).
inline void par_plan_segments(const uint8_t *sample_class, const int64_t *win_off, const ParSlab &s, ParPlan &plan, const std::vector<int64_t> &group_win)
{
    std::vector<unsigned long long> cm((size_t)(3 * ((s.n_rows + 63) / 64)), 0ull);      // the slab's class masks [word][3]
    for (int64_t k = 0; k < s.n_rows; ++k) {
        const uint8_t c = sample_class[s.r0 + k];
        if (c <= 2) cm[(size_t)(3 * (k >> 6) + c)] |= 1ull << (k & 63);
    }
    for (int64_t g = s.g_lo; g < s.g_hi; ++g) {
        const int64_t gw0 = plan.groups[(size_t)(g * PAR_GROUP_WORDS)], steps = plan.groups[(size_t)(g * PAR_GROUP_WORDS + 1)];
        plan.groups[(size_t)(g * PAR_GROUP_WORDS + 2)] = (int64_t)plan.step_off.size();
        int64_t step = 0;                   // steps of this group whose first segment is recorded
        for (int64_t w = group_win[(size_t)(2 * g)]; w < group_win[(size_t)(2 * g + 1)]; ++w) {
            const int64_t b0 = win_off[w] - s.r0, b1 = win_off[w + 1] - s.r0;
            if (b1 <= b0) continue;
            const int64_t wf = b0 >> 6, wl = (b1 - 1) >> 6;
            int64_t last = -1;
            for (int64_t k = wf; k <= wl; ++k) {
                unsigned long long m = ~0ull;
                if (k == wf) m &= ~0ull << (int)(b0 & 63);
                if (k == wl) m &= ~0ull >> (63 - (int)((b1 - 1) & 63));
                const unsigned long long s0 = cm[(size_t)(3 * k)] & m, s1 = cm[(size_t)(3 * k + 1)] & m, s2 = cm[(size_t)(3 * k + 2)] & m;
                if (!(s0 | s1 | s2)) continue;
                const int64_t at = (k - gw0) / F1X_STEP_WORDS;
                for (; step <= at; ++step) plan.step_off.push_back((int64_t)plan.segs.size() / PAR_SEG_WORDS);
                last = (int64_t)plan.segs.size();
                plan.segs.push_back(s0);
                plan.segs.push_back(s1);
                plan.segs.push_back(s2);
                plan.segs.push_back((unsigned long long)((k - gw0) % F1X_STEP_WORDS));
            }
            if (last >= 0) plan.segs[(size_t)(last + 3)] |= PAR_SEG_END;
        }
        for (; step < steps; ++step) plan.step_off.push_back((int64_t)plan.segs.size() / PAR_SEG_WORDS);
    }
}

// the whole plan of a call; step_off ends with the segment count, so step k of the plan holds segments [step_off[k], step_off[k + 1])
inline void par_plan(size_t ws_bytes, int64_t cols_pad, const uint8_t *sample_class, const int64_t *win_off, int64_t n_win, ParPlan &plan)
{
    std::vector<int64_t> group_win;
    par_plan_slabs(ws_bytes, cols_pad, win_off, n_win, plan);
    for (ParSlab &s : plan.slabs) {
        par_plan_groups(win_off, s, plan, group_win);
        par_plan_segments(sample_class, win_off, s, plan, group_win);
    }
    plan.step_off.push_back((int64_t)plan.segs.size() / PAR_SEG_WORDS);
}

// grid (tile pairs, groups of this launch): blockIdx.x counts the pairs (ta, tb) with ta <= tb row by row, blockIdx.y the groups from
// `groups` on.  out_* [ncols, ncols], zeroed before the first slab.  planes [4][cols_pad][W] of this slab, W a multiple of
// F1X_STEP_WORDS; every group's steps lie inside W.  step_off / segs: the whole tables of the plan.
__global__ void __launch_bounds__(PAR_THREADS, PAR_MIN_BLOCKS)
k_par_count(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, const int64_t *__restrict__ groups,
            const int64_t *__restrict__ step_off, const unsigned long long *__restrict__ segs, int ncols, int n_tiles, int min_win_sites,
            int32_t *__restrict__ out_score, int32_t *__restrict__ out_ntot, int32_t *__restrict__ out_wfirst, int32_t *__restrict__ out_whet)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_a[F1X_LDS_PLANES * F1X_TILE * F1X_LD];      // [plane][accession][dword]
    __shared__ __attribute__((aligned(16))) uint32_t s_b[F1X_LDS_PLANES * F1X_TILE * F1X_LD];
    int ta = 0, rest = blockIdx.x;                                  // (block-uniform) row ta of the triangle holds n_tiles - ta pairs
    while (rest >= n_tiles - ta) { rest -= n_tiles - ta; ++ta; }
    const int tb = ta + rest;
    const bool diag = ta == tb;
    const uint32_t *sb = diag ? s_a : s_b;
    const int64_t *grp = groups + (int64_t)blockIdx.y * PAR_GROUP_WORDS;
    const int64_t w0 = grp[0], steps = grp[1];
    const int64_t *soff = step_off + grp[2];
    // the lane's pairs and its staging slot: as in k_f1x_count
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    int cn[2][2] = {{0, 0}, {0, 0}}, cA[2][2] = {{0, 0}, {0, 0}}, cB[2][2] = {{0, 0}, {0, 0}}, cF[2][2] = {{0, 0}, {0, 0}};      // of the open window
    int score[2][2] = {{0, 0}, {0, 0}}, ntot[2][2] = {{0, 0}, {0, 0}}, wA[2][2] = {{0, 0}, {0, 0}}, wB[2][2] = {{0, 0}, {0, 0}}, wH[2][2] = {{0, 0}, {0, 0}};
    const int64_t row_bytes = W * 8, plane_bytes = cols_pad * row_bytes;
    const uint8_t *base = (const uint8_t *)planes;
    const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;
    const int64_t ga = (int64_t)(ta * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const int64_t gb = (int64_t)(tb * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    for (int64_t step = 0; step < steps; ++step) {
        const int64_t q0 = soff[step], q1 = soff[step + 1];          // (block-uniform) the step's segments
        if (q0 == q1) continue;                                      // no class bit in these 1024 rows: nothing to stage
        const int64_t off = step * (F1X_STEP_WORDS * 8);
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
        __syncthreads();
        for (int64_t q = q0; q < q1; ++q) {                          // a segment: one 64-bit word under a window's class masks
            const unsigned long long *sg = segs + q * PAR_SEG_WORDS;
            const unsigned long long m0 = sg[0], m1 = sg[1], m2 = sg[2], meta = sg[3];
            const unsigned long long many = m0 | m1 | m2;
            const int w = (int)(meta & (F1X_STEP_WORDS - 1));
            unsigned long long av[F1X_LDS_PLANES][2], bv[F1X_LDS_PLANES][2], ma[2], mb[2];      // [plane][x or y]
#pragma unroll
            for (int pl = 0; pl < F1X_LDS_PLANES; ++pl)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    av[pl][h] = *(const unsigned long long *)(s_a + (pl * F1X_TILE + i + 16 * h) * F1X_LD + 2 * w);
                    bv[pl][h] = *(const unsigned long long *)(sb + (pl * F1X_TILE + j + 16 * h) * F1X_LD + 2 * w);
                }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ma[h] = (av[0][h] & m0) | (av[1][h] & m1) | (av[2][h] & m2);
                mb[h] = (bv[0][h] & m0) | (bv[1][h] & m1) | (bv[2][h] & m2);
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const unsigned long long e0 = av[0][x] & bv[0][y], e1 = av[1][x] & bv[1][y];
                    const unsigned long long u = (av[2][x] & bv[2][y]) | (av[3][x] & bv[3][y]);
                    const unsigned long long ni = (av[4][x] & bv[4][y]) ^ u;
                    const unsigned long long het = ni ^ e0 ^ e1;
                    cn[x][y] += f1x_popc(ni & many);
                    cA[x][y] += f1x_popc(ni & ma[x]);
                    cB[x][y] += f1x_popc(ni & mb[y]);
                    cF[x][y] += f1x_popc((e0 & m0) | (e1 & m1) | (het & m2));
                }
            if (meta & PAR_SEG_END) {                                // (block-uniform) the window ends here
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) {
                        const int a = ta * F1X_TILE + i + 16 * x, b = tb * F1X_TILE + j + 16 * y;
                        const int n = cn[x][y], hA = cA[x][y], hB = cB[x][y], hF = cF[x][y];
                        const int hom = hA > hB ? hA : hB;
                        const bool used = n >= min_win_sites, as_f1 = hF > hom;
                        const bool a_first = hA > hB || (hA == hB && a <= b);
                        score[x][y] += used ? (as_f1 ? hF : hom) : 0;
                        ntot[x][y] += used ? n : 0;
                        wH[x][y] += used && as_f1 ? 1 : 0;
                        wA[x][y] += used && !as_f1 && a_first ? 1 : 0;
                        wB[x][y] += used && !as_f1 && !a_first ? 1 : 0;
                        cn[x][y] = cA[x][y] = cB[x][y] = cF[x][y] = 0;
                    }
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
            if (a >= ncols || b >= ncols || ntot[x][y] == 0) continue;      // a used window holds min_win_sites >= 1 rows: no total without n_tot
            const int64_t ab = (int64_t)a * ncols + b, ba = (int64_t)b * ncols + a;
            atomicAdd(out_ntot + ab, ntot[x][y]);
            if (score[x][y]) atomicAdd(out_score + ab, score[x][y]);
            if (wH[x][y]) atomicAdd(out_whet + ab, wH[x][y]);
            if (wA[x][y]) atomicAdd(out_wfirst + ab, wA[x][y]);
            if (!diag) {
                atomicAdd(out_ntot + ba, ntot[x][y]);
                if (score[x][y]) atomicAdd(out_score + ba, score[x][y]);
                if (wH[x][y]) atomicAdd(out_whet + ba, wH[x][y]);
                if (wB[x][y]) atomicAdd(out_wfirst + ba, wB[x][y]);
            }
        }
    }
}

}  // namespace snpm
