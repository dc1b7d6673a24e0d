// snpm_k_mos.hpp -- mosaic: the copying-model Viterbi (Li & Stephens with a uniform switch cost, integer costs) of every (chain, sample) over the accession columns of a panel: which accession a sample copies at every selected row.
// One of the kernel-family headers behind snpm_kernels.hpp (include that one).  It needs WAVE of snpm_k_common.hpp only and is
// launched behind k_win_planes of snpm_k_win.hpp, so that tests/mos_host_driver.cpp can compile this very text for the host
// (tests/host_kernel/): the cross-lane step is __ballot, the waves of a block meet at __syncthreads.
#pragma once

namespace snpm {
// ------------------------------------------------------------------------------------------------
// The model (include/snpmatch_hip.h, snpm_panel_mosaic, states it in full).  a: position in the column list, k: position in the
// selected rows, a chain [c0, c1) of them, S the switch cost:
//   e(a, k) = cost[class of the sample at k][canonical code of a at k], 0 without a class or with a missing call
//   V(a, c0) = e(a, c0);   k > c0:  B = min_a V(a, k - 1),  j(k - 1) = the LOWEST a that attains it,
//                                   sw(a, k) = V(a, k - 1) > B + S,   V(a, k) = min(V(a, k - 1), B + S) + e(a, k)
//   chain cost = min_a V(a, c1 - 1), state[c1 - 1] = the lowest a that attains it, state[k - 1] = sw(state[k], k) ? j(k - 1) : state[k]
//
// Two kernels per (slab of whole chains, group of samples), behind k_win_planes (planes [4][cols_pad][W]: P0, P1, P2, I; bit r of
// word w of a column is row 64 w + r of the slab):
//   k_mos_fwd<NW, T, NB>  grid (chain of the slab, sample of the group), a block of NW waves.  Thread i keeps V of the T columns
//       i T .. i T + T - 1 in registers (a thread whose run would pass ncols takes the last T columns instead and repeats its
//       neighbours' work on them: no column needs a special case in the row loop).  Per group of rows (32, a dword of a plane word;
//       fewer in the widest form) the sample's three class words (block-uniform) are
//       folded with the cost table into NB x 4 words u[b][d] = "rows whose class has bit b of its cost against code d set"; a
//       column's NB cost bit-planes are then OR_d (u[b][d] & code plane d) -- once per group, not per row.  col_cost is popcounts
//       of the same planes.  Per row: extract the NB bits, min and add, the thread's minimum (first t on ties), the wave's candidate
//       for the row's minimum by __ballot (the minimum lies in B .. B + 15 of the row before: one ballot when the copied column
//       matched, a binary search over four bits otherwise), one 32-bit key (V - B << 16 | column) per wave into LDS, ONE barrier
//       (the keys are double-buffered by row parity), the minimum key of the NW waves.  The sw bits of a column and word are one
//       64-bit word [sample][word][cols_pad]; a chain owns the words it spans (a plane word shared by two chains is two sw words), so no two
//       blocks write one word.  j and the end of the chain: one int32 per (sample, row), written by thread 0.  In the narrow
//       forms the plane dwords of the next group are loaded before the rows of the current one run: those loads do not depend on V.
//   k_mos_back  grid (chain, sample), one wave.  The path downwards: every lane follows the same (wave-uniform) walk -- the sw word
//       of the current state, its highest set bit at or below the current row, a jump to j there -- and lane r writes the state of
//       bit r of the word.  A word without a switch costs one load.
constexpr int MOS_NW_MAX = 16;               // waves of the widest block
constexpr int MOS_T_MAX = 12;                // columns per thread of the widest form
#ifndef SNPM_MOS_MAX_ACCESSIONS
#define SNPM_MOS_MAX_ACCESSIONS 12288        // MOS_NW_MAX * WAVE * MOS_T_MAX (include/snpmatch_hip.h carries the same figure)
#endif
static_assert(SNPM_MOS_MAX_ACCESSIONS == MOS_NW_MAX * WAVE * MOS_T_MAX && SNPM_MOS_MAX_ACCESSIONS <= 65536, "the widest form holds every column; a column fits the low half of a key");
constexpr int MOS_STEP_WORDS = 16;           // W of k_win_planes is a multiple of it
constexpr int64_t MOS_STEP_ROWS = (int64_t)MOS_STEP_WORDS * 64;
constexpr int MOS_CHAIN_WORDS = 4;           // int64 per chain of a slab: c0, c1 (rows of the slab), first sw word, 0
constexpr int64_t MOS_SWITCH_MAX = (int64_t)1 << 20;

// the forms of k_mos_fwd, narrowest first: the first whose NW * WAVE * T holds ncols runs
struct MosForm { int nw, t; };
constexpr MosForm MOS_FORMS[4] = {{1, 1}, {4, 1}, {4, 5}, {MOS_NW_MAX, MOS_T_MAX}};
inline int mos_form_of(int64_t ncols)
{
    int f = 0;
    while (f < 3 && (int64_t)MOS_FORMS[f].nw * WAVE * MOS_FORMS[f].t < ncols) ++f;
    return f;
}

// cost table [3][4] -> one word per cost bit: bit (4 cls + d) of bits[b] = bit b of cost[cls][d]; returns the planes needed (2 or 4)
inline int mos_cost_bits(const uint8_t *cost, uint32_t bits[4])
{
    int top = 0;
    for (int b = 0; b < 4; ++b) bits[b] = 0;
    for (int i = 0; i < 12; ++i)
        for (int b = 0; b < 4; ++b)
            if (cost[i] >> b & 1) { bits[b] |= 1u << i; if (b > top) top = b; }
    return top < 2 ? 2 : 4;
}

// sw words of a chain [c0, c1) of slab rows: the plane words it spans
__host__ __device__ __forceinline__ int64_t mos_chain_words(int64_t c0, int64_t c1) { return c1 > c0 ? ((c1 - 1) >> 6) - (c0 >> 6) + 1 : 0; }

// The host's slab plan: the run of whole chains [ch_lo, ch_hi) that starts at chain ch_lo -- as many as there are while the planes
// of their rows and ONE sample's sw words, j, class words and state fit ws_bytes, one chain at least -- and the samples of a group:
// as many as fit beside the planes, one at least.
struct MosSlab {
    int64_t ch_lo, ch_hi, r0, n_rows, W, sw_words, group;
};
inline int64_t mos_sample_bytes(int64_t cols_pad, int64_t W, int64_t sw_words, int64_t n_rows)
{
    return sw_words * cols_pad * 8 + n_rows * 8 + W * 3 * 8;         // sw; j and state; class words
}
inline MosSlab mos_slab(size_t ws_bytes, int64_t cols_pad, const int64_t *chain_off, int64_t n_chain, int64_t ch_lo, int64_t n_samples)
{
    MosSlab s;
    s.ch_lo = ch_lo; s.ch_hi = ch_lo; s.r0 = chain_off[ch_lo]; s.n_rows = 0; s.W = 0; s.sw_words = 0;
    const double budget = (double)ws_bytes;                          // (compared in fp64: no product can overflow)
    while (s.ch_hi < n_chain) {
        const int64_t n = chain_off[s.ch_hi + 1] - s.r0;
        const int64_t W = (n + MOS_STEP_ROWS - 1) / MOS_STEP_ROWS * MOS_STEP_WORDS;
        const int64_t sw = s.sw_words + mos_chain_words(chain_off[s.ch_hi] - s.r0, chain_off[s.ch_hi + 1] - s.r0);
        if (s.n_rows > 0 && n > s.n_rows && 32.0 * (double)cols_pad * (double)W + (double)mos_sample_bytes(cols_pad, W, sw, n) > budget) break;
        s.n_rows = n; s.W = W; s.sw_words = sw;
        ++s.ch_hi;
    }
    const double left = budget - 32.0 * (double)cols_pad * (double)s.W, per = (double)mos_sample_bytes(cols_pad, s.W, s.sw_words, s.n_rows);
    int64_t g = per > 0 && left > per ? (int64_t)(left / per) : 1;
    if (g > 65535) g = 65535;                                         // grid.y
    s.group = g < n_samples ? g : n_samples;
    return s;
}

__device__ __forceinline__ int mos_popc(unsigned long long v) { return __popc((uint32_t)v) + __popc((uint32_t)(v >> 32)); }

// grid (chains of the slab, samples of the group), NW * WAVE threads.  planes [4][cols_pad][W]; cls [samples][W][3] class words of
// the slab's rows (ref, alt, het); chains [n][MOS_CHAIN_WORDS]; cb: mos_cost_bits; sw [samples][sw_words][cols_pad];
// jarr [samples][n_rows]; chain_cost [samples][gridDim.x]; col_cost [samples][gridDim.x][ncols] or null.  Every sw word of a
// non-empty chain, every jarr entry of its rows, its chain_cost and col_cost cells are written; an empty chain writes nothing.
template <int NW, int T, int NB>
__global__ void __launch_bounds__(NW * WAVE)
k_mos_fwd(const unsigned long long *__restrict__ planes, int64_t cols_pad, int64_t W, const unsigned long long *__restrict__ cls,
          const int64_t *__restrict__ chains, int ncols, uint32_t cb0, uint32_t cb1, uint32_t cb2, uint32_t cb3, int32_t S,
          unsigned long long *__restrict__ sw, int64_t sw_words, int32_t *__restrict__ jarr, int64_t n_rows,
          int32_t *__restrict__ chain_cost, int32_t *__restrict__ col_cost)
{
    constexpr bool AHEAD = T <= 5;       // the narrow forms: the next half's plane dwords are loaded while this half's rows run, col_cost sums in registers
    __shared__ uint32_t s_key[2][NW];
    __shared__ uint32_t s_e[AHEAD ? 1 : T * NW * WAVE];              // the widest form: the packed cost planes of the group [t][thread], a thread's own slots
    __shared__ int32_t s_cc[AHEAD ? 1 : T * NW * WAVE];              // the widest form: col_cost sums [t][thread], a thread's own slots (its registers hold V, the cost planes and the sw bits)
    const int chain = blockIdx.x, sample = blockIdx.y;
    const int64_t c0 = chains[(int64_t)chain * MOS_CHAIN_WORDS], c1 = chains[(int64_t)chain * MOS_CHAIN_WORDS + 1];
    if (c0 >= c1) return;                                            // (block-uniform) an empty chain
    const int64_t sw0 = chains[(int64_t)chain * MOS_CHAIN_WORDS + 2];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    // The thread's T columns start at tid * T, moved down where that run would pass ncols (ncols >= T: mos_form_of): such a thread
    // repeats columns of its neighbours below -- the same values under the same column number, so whoever wins a tie names the same
    // column, and both store the same sw words and sums.  No column needs a special case in the row loop.
    const int a0 = tid * T <= ncols - T ? tid * T : ncols - T;
    // Everything below walks GROUPS of G rows inside the 64-row words: 32 (a dword of a plane word: NB registers of cost planes per
    // column) in the narrow forms; 32 / NB in the widest, which packs the NB cost planes of a group into ONE register per column
    // (a thread of 1024 has 128 registers for V, the planes and the sw bits of its twelve columns).
    constexpr int G = AHEAD ? 32 : 32 / NB, NBP = AHEAD ? NB : 1;
    constexpr uint32_t GM = AHEAD ? ~0u : (1u << (G & 31)) - 1u;
    const int64_t plane = cols_pad * W * 2;                          // dwords of a plane
    const uint32_t *planes32 = (const uint32_t *)planes;
    const uint32_t *pc = (const uint32_t *)(cls + (int64_t)sample * W * 3);
    unsigned long long *psw = sw + (int64_t)sample * sw_words * cols_pad;
    int32_t *pj = jarr + (int64_t)sample * n_rows;
    const uint32_t cbits[4] = {cb0, cb1, cb2, cb3};
    // column t of this thread is a0 + t: dwords of its plane row, a uniform stride from the thread's first
    auto col_at = [&](int t) -> int64_t { return ((int64_t)a0 + t) * W * 2; };

    int32_t V[T], cc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        V[t] = 0, cc[t] = 0;
        if (!AHEAD) s_cc[t * NW * WAVE + tid] = 0;
    }
    int32_t B = 0;                                                   // row c0: min(0, 0 + S) + e = e, and 0 > S never holds
    int buf = 0;
    const int64_t w_first = c0 >> 6, w_last = (c1 - 1) >> 6;
    // whole words: a group of the first or last word that lies outside the chain has no rows and writes zero sw bits
    const int64_t g_first = (64 / G) * w_first, g_last = (64 / G) * (w_last + 1) - 1;
    uint32_t q0[T], q1[T], q2[T], qi[T];                             // AHEAD: the plane dwords of the group the loop is at
    if (AHEAD) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const uint32_t *pt = planes32 + col_at(t) + g_first;
            q0[t] = pt[0]; q1[t] = pt[plane]; q2[t] = pt[2 * plane]; qi[t] = pt[3 * plane];
        }
    }
    for (int64_t gq = g_first; gq <= g_last; ++gq) {
        const int64_t k_lo = gq * G, hw = k_lo >> 5;                 // slab row of bit 0 of this group; its dword
        const int sh = (int)(k_lo & 31);                             // (0 in the narrow forms)
        const int r_lo = c0 > k_lo ? (c0 - k_lo < G ? (int)(c0 - k_lo) : G) : 0, r_hi = c1 - 1 - k_lo < G - 1 ? (int)(c1 - 1 - k_lo) : G - 1;
        const uint32_t in_chain = r_lo <= r_hi ? (~0u << r_lo) & (GM >> (G - 1 - r_hi)) : 0u;
        const int64_t cw = (hw >> 1) * 6 + (hw & 1);                 // class words [W][3] of two dwords
        const uint32_t k0 = pc[cw] >> sh & GM, k1 = pc[cw + 2] >> sh & GM, k2 = pc[cw + 4] >> sh & GM;
        // u[b][d]: rows of this group whose class has bit b of its cost against code d set
        uint32_t u[NB][4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int d = 0; d < 4; ++d)
                u[b][d] = ((cbits[b] >> d & 1u) ? k0 : 0u) | ((cbits[b] >> (4 + d) & 1u) ? k1 : 0u) | ((cbits[b] >> (8 + d) & 1u) ? k2 : 0u);
        uint32_t e[NBP][T];                                          // narrow: plane b of column t; widest: e[0][0] builds a column's planes, plane b at bits G b .. G b + G - 1, for s_e
#pragma unroll
        for (int t = 0; t < T; ++t) {
            uint32_t p0, p1, p2, p3;
            if (AHEAD) {
                p0 = q0[t]; p1 = q1[t]; p2 = q2[t]; p3 = qi[t];
            } else {
                const uint32_t *pt = planes32 + col_at(t) + hw;
                p0 = pt[0] >> sh; p1 = pt[plane] >> sh; p2 = pt[2 * plane] >> sh; p3 = pt[3 * plane] >> sh;     // (u holds G bits: what lies above drops out)
            }
            const uint32_t m3 = p3 & ~(p0 | p1 | p2);                // an int8 panel's "other" code: informative, none of 0 / 1 / 2
            int32_t add = 0;
#pragma unroll
            for (int i = 0; i < NBP; ++i) e[i][AHEAD ? t : 0] = 0u;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const uint32_t eb = (u[b][0] & p0) | (u[b][1] & p1) | (u[b][2] & p2) | (u[b][3] & m3);
                if (AHEAD) e[b < NBP ? b : 0][t] = eb;
                else e[0][0] |= eb << ((G * b) & 31);
                add += __popc(eb & in_chain) << b;
            }
            if (AHEAD) {
                cc[t] += add;
            } else {
                s_cc[t * NW * WAVE + tid] += add;
                s_e[t * NW * WAVE + tid] = e[0][0];
            }
        }
        if (AHEAD) {                                                 // (the last group again behind the chain's end: inside the planes, not used)
            const int64_t gn = gq < g_last ? gq + 1 : g_last;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const uint32_t *pt = planes32 + col_at(t) + gn;
                q0[t] = pt[0]; q1[t] = pt[plane]; q2[t] = pt[2 * plane]; qi[t] = pt[3 * plane];
            }
        }
        uint32_t swb[T];
#pragma unroll
        for (int t = 0; t < T; ++t) swb[t] = 0u;
        for (int r = r_lo; r <= r_hi; ++r) {
            const int32_t bs = B + S;
            int32_t lv = 0;
            int li = 0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                uint32_t ev;
                if (AHEAD) {
                    ev = (e[0][t] >> r & 1u) | ((e[NBP > 1 ? 1 : 0][t] >> r & 1u) << 1);
                    if (NB > 2) ev |= ((e[NBP > 2 ? 2 : 0][t] >> r & 1u) << 2) | ((e[NBP - 1][t] >> r & 1u) << 3);
                } else {
                    const uint32_t et = s_e[t * NW * WAVE + tid];    // (read again in every row: the barrier below keeps it out of the registers)
                    ev = (et >> r & 1u) | ((et >> ((r + G) & 31) & 1u) << 1);
                    if (NB > 2) ev |= ((et >> ((r + 2 * G) & 31) & 1u) << 2) | ((et >> ((r + 3 * G) & 31) & 1u) << 3);
                }
                const int32_t v = V[t];
                swb[AHEAD ? t : t >> 1] |= (uint32_t)(v > bs) << (AHEAD ? r : r + 16 * (t & 1));      // (the widest form: the 16 bits of two columns share a register)
                const int32_t nv = (v < bs ? v : bs) + (int32_t)ev;
                V[t] = nv;
                if (AHEAD) {
                    if (t == 0 || nv < lv) { lv = nv; li = t; }
                } else {
                    // the widest form: (V - B) << 4 | t in one minimum -- V - B <= S + 15 < 2^21 -- so that no row keeps its twelve
                    // new values and their running minima in registers until the winner's t is asked for
                    const int32_t pk = ((nv - B) << 4) | t;
                    if (t == 0 || pk < lv) lv = pk;
                }
            }
            if (!AHEAD) {
                li = lv & 15;
                lv = (lv >> 4) + B;
            }
            // The row's minimum is B + e of the column that held B in the row before: at most B + 15, and no V lies below B.  So only
            // d = V - B in 0 .. 15 can win, and one 32-bit key (d << 16 | column) per wave carries a wave's candidate: the lowest lane
            // with d == 0 where there is one (the copied column matched: nearly every row), else the lowest lane of the smallest d
            // below 16 by a binary search over its four bits with ballots, else none.
            const uint32_t d = (uint32_t)(lv - B);
            unsigned long long race = __ballot(d == 0u);
            if (!race) {
                race = __ballot(d < 16u);
                if (race) {
#pragma unroll
                    for (int b = 3; b >= 0; --b) {
                        const unsigned long long zero = __ballot(!(d >> b & 1u)) & race;
                        race = zero ? zero : race;
                    }
                }
            }
            if (race ? lane == __builtin_ctzll(race) : lane == 0) s_key[buf][wave] = race ? (d << 16) | (uint32_t)(a0 + li) : ~0u;
            __syncthreads();
            uint32_t key = s_key[buf][0];
#pragma unroll
            for (int x = 1; x < NW; ++x) {
                const uint32_t o = s_key[buf][x];
                key = o < key ? o : key;
            }
            buf ^= 1;
            B += (int32_t)(key >> 16);
            if (tid == 0) pj[k_lo + r] = (int32_t)(key & 0xFFFFu);
        }
        // the G sw bits of every column of this thread, at their place in the chain's own copy of the word
#pragma unroll
        for (int t = 0; t < T; ++t)
            {
                unsigned long long *word = psw + (sw0 + ((k_lo >> 6) - w_first)) * cols_pad + a0 + t;
                if (AHEAD) ((uint32_t *)word)[hw & 1] = swb[t];
                else if (G == 16) ((uint16_t *)word)[(k_lo >> 4) & 3] = (uint16_t)(swb[t >> 1] >> (16 * (t & 1)));
                else ((uint8_t *)word)[(k_lo >> 3) & 7] = (uint8_t)(swb[t >> 1] >> (16 * (t & 1)));
            }
    }
    if (tid == 0) chain_cost[(int64_t)sample * gridDim.x + chain] = B;
    if (col_cost) {
#pragma unroll
        for (int t = 0; t < T; ++t)
            col_cost[((int64_t)sample * gridDim.x + chain) * ncols + a0 + t] = AHEAD ? cc[t] : s_cc[t * NW * WAVE + tid];
    }
}

// grid (chains of the slab, samples of the group), WAVE threads.  state [samples][n_rows]: every row of a non-empty chain is written.
__global__ void __launch_bounds__(WAVE)
k_mos_back(const unsigned long long *__restrict__ sw, int64_t sw_words, int64_t cols_pad, const int32_t *__restrict__ jarr, int64_t n_rows,
           const int64_t *__restrict__ chains, int32_t *__restrict__ state)
{
    const int chain = blockIdx.x, sample = blockIdx.y, lane = threadIdx.x;
    const int64_t c0 = chains[(int64_t)chain * MOS_CHAIN_WORDS], c1 = chains[(int64_t)chain * MOS_CHAIN_WORDS + 1];
    if (c0 >= c1) return;
    const int64_t sw0 = chains[(int64_t)chain * MOS_CHAIN_WORDS + 2];
    const unsigned long long *psw = sw + (int64_t)sample * sw_words * cols_pad;
    const int32_t *pj = jarr + (int64_t)sample * n_rows;
    int32_t *ps = state + (int64_t)sample * n_rows;
    const int64_t w_first = c0 >> 6, w_last = (c1 - 1) >> 6;
    int32_t st = pj[c1 - 1];
    for (int64_t w = w_last; w >= w_first; --w) {
        const int lo = w == w_first ? (int)(c0 & 63) : 0;
        int cur = w == w_last ? (int)((c1 - 1) & 63) : 63;           // bits lo .. cur of this word are still to be written
        while (cur >= lo) {
            // (bit c0 of the first word and every bit outside the chain are zero: a set bit b has a row b - 1 inside the chain)
            const unsigned long long x = psw[(sw0 + (w - w_first)) * cols_pad + st] & (~0ull >> (63 - cur));
            const int b = x ? 63 - __builtin_clzll(x) : lo;          // rows b .. cur keep st
            if (lane >= b && lane <= cur) ps[w * 64 + lane] = st;
            if (!x) break;
            // sw(st, b): row b - 1 is j(b - 1) -- it may lie in the previous word
            st = pj[w * 64 + b - 1];
            cur = b - 1;
        }
    }
}

}  // namespace snpm
