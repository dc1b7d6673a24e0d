// snpm_k_ibd.hpp -- ibd: for EVERY pair of accession columns, the genome windows in which the two are identical (shared haplotype segments, identity by descent), and the runs those windows form along a chromosome.
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp, k_win_planes of
// snpm_k_win.hpp (its planes) and the constants and f1x_popc of snpm_k_f1x.hpp only, so that tests/ibd_host_driver.cpp can compile
// this very text for the host (tests/host_kernel/).  The plan functions below are plain host code.
#pragma once
#include <cstdint>
#include <vector>

namespace snpm {
// ------------------------------------------------------------------------------------------------
// Columns a, b (positions in the column list), canonical codes (kin_code), windows [win_off[w], win_off[w + 1]) of the selected
// rows.  Per cell (a, b) and window:
//   n = #rows where both codes are homozygous (0 or 1)        d = #rows among those where the two codes differ
// (hom_same + hom_diff and hom_diff of snpm_k_win.hpp's pair cells).  Hets, code 3 and missing calls count nowhere.  With
// min_win_sites >= 1 and 0 <= max_diff_ppm <= 1 000 000 a window is
//   used    iff n >= min_win_sites
//   shared  iff used and d * 1 000 000 <= max_diff_ppm * n        (64-bit integers; d <= n < 2^31)
//   a break iff used and not shared
// and the windows of a call, scanned in order, form RUNS: a maximal set of shared windows without a break between two consecutive
// members.  Unused windows neither break a run nor count in it; a run's length is its number of shared windows; a run is reported
// when its length is at least min_run >= 1.  Seven int32 matrices [ncols][ncols], full and symmetric -- w_used, w_shared, n_shared
// (sum of n over shared windows), d_shared, run_max, n_runs (reported runs), w_in_runs (shared windows inside reported runs) --
// and two bitsets used / shared, uint32 [ncols][ncols][wwords], wwords = ceil(n_win / 32): window w is bit w % 32 of word w / 32.
//
// Per SLAB of WHOLE windows (ibd_plan: the planes of a slab fit a workspace budget, at least one window whatever the budget):
//   planes  k_win_planes AS IT STANDS, `first` = the slab's first selected row; only P0 and P1 are read afterwards.
//   segments  a SEGMENT is (mask, meta): a window's bit range inside one 64-bit word, and the word's place in its LDS step, an "ends
//       a window" flag and the window's index in the call.  Every word a window touches gives a segment, whatever the planes hold:
//       a window with rows always has its segments, its last one carries the flag; an empty window has none and stays unused.
//   k_ibd_count  the tiling of k_par_count -- F1X_TILE x F1X_TILE pairs per block of 256 threads, a 2 x 2 register tile per lane, a
//       GROUP of whole consecutive windows per blockIdx.y -- with TWO planes per side staged per step: H = P0 | P1 (made while
//       staging) and P1.  Per pair and segment
//         h = Ha & Hb & M        n += popc(h)        d += popc(h & (P1a ^ P1b))
//       -- inside h both codes are 0 or 1, so they differ exactly where the P1 bits differ: h & (P1a ^ P1b) IS
//       ((P0a & P1b) | (P1a & P0b)) & M.  At a segment that ends a window (block-uniform branch) the lane applies the two integer
//       rules, adds into its four totals, sets the window's bit in two lane-local 32-bit words and clears n and d.  The bit words
//       go out with atomicOr when the window index enters the next 32-window word and at the end of the group: one atomic per
//       (cell, bit word, group) at most (zero words are skipped).  The totals go into the zeroed matrices with int32 atomicAdd,
//       zero totals skipped.  A block off the diagonal writes both mirror cells; a diagonal block holds (a, b) and (b, a) as pairs
//       of its own and writes only its own cells.  No window is split between groups or slabs, so every (cell, window) is
//       evaluated by exactly one block and the results do not depend on the schedule.
//   k_ibd_runs  once, after the last slab: a thread per cell walks the cell's wwords words of both bitsets in window order and
//       writes run_max, n_runs, w_in_runs.  No atomics, every cell written.
constexpr int IBD_THREADS = F1X_THREADS;
constexpr int IBD_MIN_BLOCKS = 5;           // blocks per CU the register budget is set for (__launch_bounds__): the kernel takes 84 VGPRs unconstrained, which the register file holds five times (at most 96); asked for six it spills
constexpr int IBD_LDS_PLANES = 2;           // planes in LDS: H = P0 | P1, P1
constexpr int IBD_SEG_WORDS = 2;            // 64-bit words of a segment: mask, meta
constexpr unsigned long long IBD_SEG_END = 16ull;      // meta: bits 0..3 the word inside its step, bit 4 "ends a window", bits 8.. the window's index
constexpr int IBD_SEG_WIN_SHIFT = 8;
constexpr int IBD_GROUP_WORDS = 3;          // int64 per group: first word (step-aligned, in the slab's planes), steps, index of its first step in step_off
constexpr int64_t IBD_MAX_GRID_Y = 65535;   // groups per launch
constexpr int IBD_RUN_THREADS = 256;        // k_ibd_runs: cells per block
constexpr long long IBD_PPM = 1000000;
static_assert(F1X_STEP_WORDS == 16, "the word inside a step is four bits of meta");

struct IbdSlab {
    int64_t w_lo, w_hi;     // windows [w_lo, w_hi)
    int64_t r0, n_rows;     // selected rows [r0, r0 + n_rows): bits 0 .. n_rows - 1 of the slab's plane rows
    int64_t W;              // words per plane row: whole steps
    int64_t g_lo, g_hi;     // groups [g_lo, g_hi)
};

struct IbdPlan {
    std::vector<IbdSlab> slabs;                 // slabs without a row are not listed
    std::vector<int64_t> groups;                // [n_groups][IBD_GROUP_WORDS]
    std::vector<int64_t> step_off;              // per step of every group, in group order: its first segment; one closing entry
    std::vector<unsigned long long> segs;       // [n_segs][IBD_SEG_WORDS]
    int64_t max_W = 0, max_rows = 0;            // of the largest slab
};

__host__ __device__ __forceinline__ int64_t ibd_words(int64_t n_rows) { return (n_rows + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS * F1X_STEP_WORDS; }

// Slabs: whole windows while the planes [4][cols_pad][W] fit ws_bytes, at least one window with rows whatever the budget (compared
// in fp64: no product can overflow).  Empty windows ride with their neighbours.
inline void ibd_plan_slabs(size_t ws_bytes, int64_t cols_pad, const int64_t *win_off, int64_t n_win, IbdPlan &plan)
{
    const double word_bytes = (double)F1X_PLANES * (double)cols_pad * 8.0;
    int64_t w = 0;
    while (w < n_win) {
        IbdSlab s;
        s.w_lo = w;
        s.r0 = win_off[w];
        int64_t rows = 0;
        while (w < n_win) {
            const int64_t more = win_off[w + 1] - s.r0;
            if (rows > 0 && more > rows && (double)ibd_words(more) * word_bytes > (double)ws_bytes) break;
            rows = more;
            ++w;
        }
        s.w_hi = w;
        s.n_rows = rows;
        s.W = ibd_words(rows);
        s.g_lo = s.g_hi = 0;
        if (rows == 0) continue;
        if (s.W > plan.max_W) plan.max_W = s.W;
        if (rows > plan.max_rows) plan.max_rows = rows;
        plan.slabs.push_back(s);
    }
}

// Groups of a slab: whole consecutive windows while their bit span stays within F1X_CHUNK_WORDS words; a longer window is a group
// of its own.  A group's steps are the step-aligned run of words covering its bits.  Windows without a row join no group.
// The group table gets (first word, steps, 0); ibd_plan_segments fills the third entry.
inline void ibd_plan_groups(const int64_t *win_off, IbdSlab &s, IbdPlan &plan, std::vector<int64_t> &group_win)
{
    const int64_t chunk_rows = (int64_t)F1X_CHUNK_WORDS * 64;
    s.g_lo = (int64_t)plan.groups.size() / IBD_GROUP_WORDS;
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
    s.g_hi = (int64_t)plan.groups.size() / IBD_GROUP_WORDS;
}

// Segments of the groups [s.g_lo, s.g_hi) of a slab, whose windows are group_win[2 g], group_win[2 g + 1] (g counted over the plan):
// one per (window with rows, word it touches), in window order.
inline void ibd_plan_segments(const int64_t *win_off, const IbdSlab &s, IbdPlan &plan, const std::vector<int64_t> &group_win)
{
    for (int64_t g = s.g_lo; g < s.g_hi; ++g) {
        const int64_t gw0 = plan.groups[(size_t)(g * IBD_GROUP_WORDS)], steps = plan.groups[(size_t)(g * IBD_GROUP_WORDS + 1)];
        plan.groups[(size_t)(g * IBD_GROUP_WORDS + 2)] = (int64_t)plan.step_off.size();
        int64_t step = 0;                   // steps of this group whose first segment is recorded
        for (int64_t w = group_win[(size_t)(2 * g)]; w < group_win[(size_t)(2 * g + 1)]; ++w) {
            const int64_t b0 = win_off[w] - s.r0, b1 = win_off[w + 1] - s.r0;
            if (b1 <= b0) continue;
            const int64_t wf = b0 >> 6, wl = (b1 - 1) >> 6;
            for (int64_t k = wf; k <= wl; ++k) {
                unsigned long long m = ~0ull;
                if (k == wf) m &= ~0ull << (int)(b0 & 63);
                if (k == wl) m &= ~0ull >> (63 - (int)((b1 - 1) & 63));
                const int64_t at = (k - gw0) / F1X_STEP_WORDS;
                for (; step <= at; ++step) plan.step_off.push_back((int64_t)plan.segs.size() / IBD_SEG_WORDS);
                plan.segs.push_back(m);
                plan.segs.push_back((unsigned long long)((k - gw0) % F1X_STEP_WORDS) | (k == wl ? IBD_SEG_END : 0ull) |
                                    ((unsigned long long)w << IBD_SEG_WIN_SHIFT));
            }
        }
        for (; step < steps; ++step) plan.step_off.push_back((int64_t)plan.segs.size() / IBD_SEG_WORDS);
    }
}

// the whole plan of a call; step_off ends with the segment count, so step k of the plan holds segments [step_off[k], step_off[k + 1])
inline void ibd_plan(size_t ws_bytes, int64_t cols_pad, const int64_t *win_off, int64_t n_win, IbdPlan &plan)
{
    std::vector<int64_t> group_win;
    ibd_plan_slabs(ws_bytes, cols_pad, win_off, n_win, plan);
    for (IbdSlab &s : plan.slabs) {
        ibd_plan_groups(win_off, s, plan, group_win);
        ibd_plan_segments(win_off, s, plan, group_win);
    }
    plan.step_off.push_back((int64_t)plan.segs.size() / IBD_SEG_WORDS);
}

// the lane's bit words of bit word `word` into the two bitsets (both mirror cells off the diagonal), then cleared
__device__ __forceinline__ void ibd_flush_bits(uint32_t (&ub)[2][2], uint32_t (&sb)[2][2], int64_t word, int64_t wwords, int ta, int tb, int i, int j, int ncols,
                                               bool diag, uint32_t *__restrict__ used_bits, uint32_t *__restrict__ shared_bits)
{
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int a = ta * F1X_TILE + i + 16 * x;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int b = tb * F1X_TILE + j + 16 * y;
            const uint32_t u = ub[x][y], s = sb[x][y];
            ub[x][y] = sb[x][y] = 0u;
            if (a >= ncols || b >= ncols || u == 0u) continue;              // a shared window is a used one: no shared bit without a used bit
            const int64_t ab = ((int64_t)a * ncols + b) * wwords + word, ba = ((int64_t)b * ncols + a) * wwords + word;
            atomicOr(used_bits + ab, u);
            if (s) atomicOr(shared_bits + ab, s);
            if (!diag) {
                atomicOr(used_bits + ba, u);
                if (s) atomicOr(shared_bits + ba, s);
            }
        }
    }
}

// grid (tile pairs, groups of this launch): blockIdx.x counts the pairs (ta, tb) with ta <= tb row by row, blockIdx.y the groups from
// `groups` on.  out_* [ncols, ncols] and the bitsets [ncols, ncols, wwords], zeroed before the first slab.  planes [4][cols_pad][W] of
// this slab, W a multiple of F1X_STEP_WORDS; every group's steps lie inside W.  step_off / segs: the whole tables of the plan.
__global__ void __launch_bounds__(IBD_THREADS, IBD_MIN_BLOCKS)
k_ibd_count(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, const int64_t *__restrict__ groups,
            const int64_t *__restrict__ step_off, const unsigned long long *__restrict__ segs, int ncols, int n_tiles, int min_win_sites,
            int max_diff_ppm, int64_t wwords, int32_t *__restrict__ out_wused, int32_t *__restrict__ out_wshared, int32_t *__restrict__ out_nshared,
            int32_t *__restrict__ out_dshared, uint32_t *__restrict__ used_bits, uint32_t *__restrict__ shared_bits)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_a[IBD_LDS_PLANES * F1X_TILE * F1X_LD];      // [plane][accession][dword]
    __shared__ __attribute__((aligned(16))) uint32_t s_b[IBD_LDS_PLANES * F1X_TILE * F1X_LD];
    int ta = 0, rest = blockIdx.x;                                  // (block-uniform) row ta of the triangle holds n_tiles - ta pairs
    while (rest >= n_tiles - ta) { rest -= n_tiles - ta; ++ta; }
    const int tb = ta + rest;
    const bool diag = ta == tb;
    const uint32_t *sb = diag ? s_a : s_b;
    const int64_t *grp = groups + (int64_t)blockIdx.y * IBD_GROUP_WORDS;
    const int64_t w0 = grp[0], steps = grp[1];
    const int64_t *soff = step_off + grp[2];
    // the lane's pairs and its staging slot: as in k_f1x_count
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    int cn[2][2] = {{0, 0}, {0, 0}}, cd[2][2] = {{0, 0}, {0, 0}};                                   // of the open window
    int wu[2][2] = {{0, 0}, {0, 0}}, ws[2][2] = {{0, 0}, {0, 0}}, ns[2][2] = {{0, 0}, {0, 0}}, ds[2][2] = {{0, 0}, {0, 0}};
    uint32_t ubits[2][2] = {{0u, 0u}, {0u, 0u}}, sbits[2][2] = {{0u, 0u}, {0u, 0u}};                // of bit word `cur`
    int64_t cur = -1;                                                // (block-uniform) the bit word the lane-local words stand for
    const int64_t row_bytes = W * 8, plane_bytes = cols_pad * row_bytes;
    const uint8_t *base = (const uint8_t *)planes;
    const int srow = threadIdx.x >> 3, sslot = threadIdx.x & 7;
    const int64_t ga = (int64_t)(ta * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    const int64_t gb = (int64_t)(tb * F1X_TILE + srow) * row_bytes + w0 * 8 + 16 * sslot;
    for (int64_t step = 0; step < steps; ++step) {
        const int64_t q0 = soff[step], q1 = soff[step + 1];          // (block-uniform) the step's segments
        if (q0 == q1) continue;
        const int64_t off = step * (F1X_STEP_WORDS * 8);
        {
            const uint4 v0 = *(const uint4 *)(base + ga + off), v1 = *(const uint4 *)(base + ga + plane_bytes + off);
            uint4 h;
            h.x = v0.x | v1.x; h.y = v0.y | v1.y; h.z = v0.z | v1.z; h.w = v0.w | v1.w;
            uint32_t *dst = s_a + srow * F1X_LD + 4 * sslot;
            *(uint4 *)(dst) = h;
            *(uint4 *)(dst + F1X_TILE * F1X_LD) = v1;
        }
        if (!diag) {
            const uint4 v0 = *(const uint4 *)(base + gb + off), v1 = *(const uint4 *)(base + gb + plane_bytes + off);
            uint4 h;
            h.x = v0.x | v1.x; h.y = v0.y | v1.y; h.z = v0.z | v1.z; h.w = v0.w | v1.w;
            uint32_t *dst = s_b + srow * F1X_LD + 4 * sslot;
            *(uint4 *)(dst) = h;
            *(uint4 *)(dst + F1X_TILE * F1X_LD) = v1;
        }
        __syncthreads();
        for (int64_t q = q0; q < q1; ++q) {                          // a segment: one 64-bit word under a window's bit range
            const unsigned long long *sg = segs + q * IBD_SEG_WORDS;
            const unsigned long long m = sg[0], meta = sg[1];
            const int w = (int)(meta & (F1X_STEP_WORDS - 1));
            unsigned long long ah[2], a1[2], bh[2], b1[2];           // [x or y]
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ah[h] = *(const unsigned long long *)(s_a + (i + 16 * h) * F1X_LD + 2 * w) & m;
                a1[h] = *(const unsigned long long *)(s_a + (F1X_TILE + i + 16 * h) * F1X_LD + 2 * w);
                bh[h] = *(const unsigned long long *)(sb + (j + 16 * h) * F1X_LD + 2 * w);
                b1[h] = *(const unsigned long long *)(sb + (F1X_TILE + j + 16 * h) * F1X_LD + 2 * w);
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const unsigned long long h = ah[x] & bh[y];
                    cn[x][y] += f1x_popc(h);
                    cd[x][y] += f1x_popc(h & (a1[x] ^ b1[y]));
                }
            if (meta & IBD_SEG_END) {                                // (block-uniform) the window ends here
                const int64_t win = (int64_t)(meta >> IBD_SEG_WIN_SHIFT);
                if ((win >> 5) != cur) {                             // (block-uniform) the window index enters another bit word
                    if (cur >= 0) ibd_flush_bits(ubits, sbits, cur, wwords, ta, tb, i, j, ncols, diag, used_bits, shared_bits);
                    cur = win >> 5;
                }
                const uint32_t bit = 1u << (int)(win & 31);
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) {
                        const int n = cn[x][y], d = cd[x][y];
                        const bool used = n >= min_win_sites;
                        const bool shared = used && (long long)d * IBD_PPM <= (long long)max_diff_ppm * (long long)n;
                        wu[x][y] += used ? 1 : 0;
                        ws[x][y] += shared ? 1 : 0;
                        ns[x][y] += shared ? n : 0;
                        ds[x][y] += shared ? d : 0;
                        ubits[x][y] |= used ? bit : 0u;
                        sbits[x][y] |= shared ? bit : 0u;
                        cn[x][y] = cd[x][y] = 0;
                    }
            }
        }
        __syncthreads();
    }
    if (cur >= 0) ibd_flush_bits(ubits, sbits, cur, wwords, ta, tb, i, j, ncols, diag, used_bits, shared_bits);
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int a = ta * F1X_TILE + i + 16 * x;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int b = tb * F1X_TILE + j + 16 * y;
            if (a >= ncols || b >= ncols || wu[x][y] == 0) continue;       // no shared window without a used one
            const int64_t ab = (int64_t)a * ncols + b, ba = (int64_t)b * ncols + a;
            atomicAdd(out_wused + ab, wu[x][y]);
            if (ws[x][y]) atomicAdd(out_wshared + ab, ws[x][y]);
            if (ns[x][y]) atomicAdd(out_nshared + ab, ns[x][y]);
            if (ds[x][y]) atomicAdd(out_dshared + ab, ds[x][y]);
            if (!diag) {
                atomicAdd(out_wused + ba, wu[x][y]);
                if (ws[x][y]) atomicAdd(out_wshared + ba, ws[x][y]);
                if (ns[x][y]) atomicAdd(out_nshared + ba, ns[x][y]);
                if (ds[x][y]) atomicAdd(out_dshared + ba, ds[x][y]);
            }
        }
    }
}

// grid (ceil(cells / IBD_RUN_THREADS)): thread t of the launch takes cell t of the `cells` = ncols * ncols cells.  The bitsets as
// k_ibd_count left them after the last slab; bits at and above n_win are zero, so the words are walked whole.  Walks the USED
// windows of the cell in order: a shared one lengthens the open run, any other (a break) closes it.
__global__ void __launch_bounds__(IBD_RUN_THREADS)
k_ibd_runs(const uint32_t *__restrict__ used_bits, const uint32_t *__restrict__ shared_bits, int64_t cells, int64_t wwords, int min_run,
           int32_t *__restrict__ out_runmax, int32_t *__restrict__ out_nruns, int32_t *__restrict__ out_winruns)
{
    const int64_t cell = (int64_t)blockIdx.x * IBD_RUN_THREADS + threadIdx.x;
    if (cell >= cells) return;
    const uint32_t *ub = used_bits + cell * wwords, *sb = shared_bits + cell * wwords;
    int len = 0, run_max = 0, n_runs = 0, w_in = 0;
    for (int64_t k = 0; k < wwords; ++k) {
        uint32_t u = ub[k];
        const uint32_t s = sb[k];
        while (u) {
            const uint32_t bit = u & (0u - u);                       // the lowest used window of the word
            u ^= bit;
            if (s & bit) { ++len; continue; }
            run_max = len > run_max ? len : run_max;
            n_runs += len >= min_run ? 1 : 0;
            w_in += len >= min_run ? len : 0;
            len = 0;
        }
    }
    run_max = len > run_max ? len : run_max;                         // the run still open at the last window (len 0: nothing, min_run >= 1)
    n_runs += len >= min_run ? 1 : 0;
    w_in += len >= min_run ? len : 0;
    out_runmax[cell] = run_max;
    out_nruns[cell] = n_runs;
    out_winruns[cell] = w_in;
}

}  // namespace snpm
