// snpm_api_mos.hpp -- C ABI: mosaic -- the copying-model Viterbi path of every (chain, sample) over the accession columns of the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- mosaic
// As snpm_panel_parent_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row and
// column index lying inside the panel, on a sound chain_off and on 15 * (longest chain) + S < 2^31 (V never wraps).
//
// Slabs: mos_slab of snpm_k_mos.hpp cuts the chain axis into runs of WHOLE chains whose planes fit the workspace budget
// (SNPM_MOS_WS_MB) beside one sample's sw words, j, class words and states; a chain larger than the budget is a slab of its own.  The
// samples of a slab are taken in groups of as many as fit beside the planes.  k_win_planes runs once per slab, k_mos_fwd and
// k_mos_back once per (slab, group); every chain is computed whole by one block, so the result does not depend on the budget.
int snpm_panel_mosaic(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                      const int64_t *chain_off, int64_t n_chain, const uint8_t *sample_class, int64_t n_samples, const uint8_t *cost,
                      int32_t switch_cost, int32_t *state, int32_t *chain_cost, int32_t *col_cost)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0 && n_chain >= 0 && n_samples >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_MOS_MAX_ACCESSIONS, "too many accessions for one call (SNPM_MOS_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more");
    CHECK_ARG(ctx, n_chain <= SNPM_MOS_MAX_CHAINS, "too many chains for one call (SNPM_MOS_MAX_CHAINS)");
    if (int bad = check_offsets(ctx, "chain_off", chain_off, n_chain, n_rows)) return bad;
    const bool work = ncols > 0 && n_rows > 0;
    if (work) CHECK_ARG(ctx, n_samples >= 1, "n_samples must be at least 1");
    CHECK_ARG(ctx, cost != nullptr, "cost is NULL");
    for (int i = 0; i < 12; ++i) CHECK_ARG(ctx, cost[i] <= 15, "cost holds an entry above 15");
    CHECK_ARG(ctx, switch_cost >= 1 && (int64_t)switch_cost <= MOS_SWITCH_MAX, "switch_cost must be 1 .. 2^20");
    int64_t longest = 0;
    for (int64_t c = 0; c < n_chain; ++c) longest = std::max(longest, chain_off[c + 1] - chain_off[c]);
    CHECK_ARG(ctx, 15 * longest + (int64_t)switch_cost <= INT32_MAX, "15 * (longest chain) + switch_cost must stay below 2^31");
    if (n_rows > 0 && n_samples > 0) {
        CHECK_ARG(ctx, sample_class != nullptr, "sample_class is NULL");
        for (int64_t k = 0, n = n_samples * n_rows; k < n; ++k)
            CHECK_ARG(ctx, sample_class[k] <= 2 || sample_class[k] == 0xFF, "sample_class holds a byte other than 0, 1, 2 or 0xFF");
    }
    if (ncols > 0 && n_samples > 0) {
        if (n_rows > 0) CHECK_ARG(ctx, state != nullptr, "state is NULL");
        if (n_chain > 0) CHECK_ARG(ctx, chain_cost != nullptr, "chain_cost is NULL");
    }
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0 || n_samples == 0) return SNPM_OK;                // nothing to write, nothing launched
    // empty chains, and every chain of a call without rows, cost nothing
    if (n_chain > 0) memset(chain_cost, 0, (size_t)n_samples * (size_t)n_chain * sizeof(int32_t));
    if (col_cost && n_chain > 0) memset(col_cost, 0, (size_t)n_samples * (size_t)n_chain * (size_t)ncols * sizeof(int32_t));
    if (n_rows == 0) return SNPM_OK;                                 // zero costs, nothing launched
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t cols_pad = (ncols + WN_PL_COLS - 1) / WN_PL_COLS * WN_PL_COLS;
    uint32_t cb[4];
    const int nb = mos_cost_bits(cost, cb);
    const int form = mos_form_of(ncols);
    // the plan, and the largest of everything over its slabs: the workspaces are sized once, before the first launch
    std::vector<MosSlab> slabs;
    MosSlab top = {0, 0, 0, 0, 0, 0, 0};
    int64_t top_chains = 0, top_sw = 0, top_rows_g = 0, top_cls = 0, top_cc = 0;
    for (int64_t ch = 0; ch < n_chain;) {
        const MosSlab s = mos_slab(ctx->mos_ws_bytes, cols_pad, chain_off, n_chain, ch, n_samples);
        ch = s.ch_hi;
        if (s.n_rows == 0) continue;                                 // (trailing empty chains)
        slabs.push_back(s);
        top.n_rows = std::max(top.n_rows, s.n_rows);
        top.W = std::max(top.W, s.W);
        top_chains = std::max(top_chains, s.ch_hi - s.ch_lo);
        top_sw = std::max(top_sw, s.group * s.sw_words);
        top_rows_g = std::max(top_rows_g, s.group * s.n_rows);
        top_cls = std::max(top_cls, s.group * s.W * 3);
        top_cc = std::max(top_cc, s.group * (s.ch_hi - s.ch_lo));
    }
    Scratch sc;     // bit-planes [4][cols_pad][W] of a slab of whole chains; sw words, j | state and class words of a group of samples; chain table; chain_cost | col_cost; column list; row list
    unsigned long long *d_planes, *d_sw, *d_cls;
    int32_t *d_j, *d_cost, *d_cols = nullptr;
    int64_t *d_chains, *d_rowlist = nullptr;
    sc.want(d_planes, (size_t)(4 * cols_pad * top.W));
    sc.want(d_sw, (size_t)top_sw * (size_t)cols_pad);
    sc.want(d_j, (size_t)top_rows_g * 2);
    sc.want(d_cls, (size_t)top_cls);
    sc.want(d_chains, (size_t)top_chains * MOS_CHAIN_WORDS);
    sc.want(d_cost, (size_t)top_cc * (size_t)(1 + (col_cost ? ncols : 0)));
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(top.n_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    std::vector<int64_t> h_chains;
    std::vector<unsigned long long> h_cls;
    for (const MosSlab &s : slabs) {
        const int64_t n_ch = s.ch_hi - s.ch_lo;
        h_chains.assign((size_t)n_ch * MOS_CHAIN_WORDS, 0);
        int64_t swb = 0;
        for (int64_t c = 0; c < n_ch; ++c) {
            const int64_t c0 = chain_off[s.ch_lo + c] - s.r0, c1 = chain_off[s.ch_lo + c + 1] - s.r0;
            h_chains[(size_t)c * MOS_CHAIN_WORDS] = c0;
            h_chains[(size_t)c * MOS_CHAIN_WORDS + 1] = c1;
            h_chains[(size_t)c * MOS_CHAIN_WORDS + 2] = swb;
            swb += mos_chain_words(c0, c1);
        }
        HIPCHK(ctx, hipMemcpyAsync(d_chains, h_chains.data(), h_chains.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        // the planes of the slab's rows: the shared walk, over this slab alone
        rc = for_each_row_slab(ctx, row_idx ? row_idx + s.r0 : nullptr, d_rowlist, row0 + s.r0, s.n_rows, s.n_rows,
                               [&](const int64_t *d_rows, int64_t first, int64_t, int64_t n_valid) {
            ProfScope ps(ctx, PK_WIN_P);
            const dim3 grid((unsigned)s.W, (unsigned)(cols_pad / WN_PL_COLS));
            hipLaunchKernelGGL(k_win_planes, grid, dim3(WN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows, first,
                               n_valid, d_cols, ncols, d_planes, cols_pad, s.W);
            HIPCHK(ctx, hipGetLastError());
            return (int)SNPM_OK;
        });
        if (rc) return rc;
        for (int64_t g0 = 0; g0 < n_samples; g0 += s.group) {
            const int64_t g = std::min(s.group, n_samples - g0);
            int32_t *d_state = d_j + g * s.n_rows, *d_cc = col_cost ? d_cost + g * n_ch : nullptr;
            h_cls.assign((size_t)(g * s.W * 3), 0ull);
            for (int64_t i = 0; i < g; ++i) {
                const uint8_t *c = sample_class + (g0 + i) * n_rows + s.r0;
                unsigned long long *m = h_cls.data() + i * s.W * 3;
                for (int64_t k = 0; k < s.n_rows; ++k)
                    if (c[k] <= 2) m[(k >> 6) * 3 + c[k]] |= 1ull << (k & 63);
            }
            HIPCHK(ctx, hipMemcpyAsync(d_cls, h_cls.data(), h_cls.size() * 8, hipMemcpyHostToDevice, ctx->stream));
            // (an empty chain's cells are not written by the kernels)
            HIPCHK(ctx, hipMemsetAsync(d_cost, 0, (size_t)(g * n_ch) * (size_t)(1 + (col_cost ? ncols : 0)) * sizeof(int32_t), ctx->stream));
            const dim3 grid((unsigned)n_ch, (unsigned)g);
            {
                ProfScope ps(ctx, PK_MOS_F);
#define MOS_FWD_NB(NW, T, NB)                                                                                                       \
    hipLaunchKernelGGL((k_mos_fwd<NW, T, NB>), grid, dim3(NW * WAVE), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, s.W,    \
                       (const unsigned long long *)d_cls, (const int64_t *)d_chains, (int)ncols, cb[0], cb[1], cb[2], cb[3], switch_cost, d_sw,  \
                       s.sw_words, d_j, s.n_rows, d_cost, d_cc)
#define MOS_FWD(NW, T) do { if (nb == 2) MOS_FWD_NB(NW, T, 2); else MOS_FWD_NB(NW, T, 4); } while (0)
                switch (form) {
                case 0: MOS_FWD(MOS_FORMS[0].nw, MOS_FORMS[0].t); break;
                case 1: MOS_FWD(MOS_FORMS[1].nw, MOS_FORMS[1].t); break;
                case 2: MOS_FWD(MOS_FORMS[2].nw, MOS_FORMS[2].t); break;
                default: MOS_FWD(MOS_FORMS[3].nw, MOS_FORMS[3].t); break;
                }
#undef MOS_FWD
#undef MOS_FWD_NB
                HIPCHK(ctx, hipGetLastError());
            }
            {
                ProfScope ps(ctx, PK_MOS_B);
                hipLaunchKernelGGL(k_mos_back, grid, dim3(WAVE), 0, ctx->stream, (const unsigned long long *)d_sw, s.sw_words, cols_pad,
                                   (const int32_t *)d_j, s.n_rows, (const int64_t *)d_chains, d_state);
                HIPCHK(ctx, hipGetLastError());
            }
            // every row of the slab lies in a non-empty chain: the whole [g][n_rows] block of states was written
            HIPCHK(ctx, hipMemcpy2DAsync(state + g0 * n_rows + s.r0, (size_t)n_rows * 4, d_state, (size_t)s.n_rows * 4, (size_t)s.n_rows * 4, (size_t)g,
                                         hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipMemcpy2DAsync(chain_cost + g0 * n_chain + s.ch_lo, (size_t)n_chain * 4, d_cost, (size_t)n_ch * 4, (size_t)n_ch * 4, (size_t)g,
                                         hipMemcpyDeviceToHost, ctx->stream));
            if (col_cost)
                HIPCHK(ctx, hipMemcpy2DAsync(col_cost + (g0 * n_chain + s.ch_lo) * ncols, (size_t)(n_chain * ncols) * 4, d_cc, (size_t)(n_ch * ncols) * 4,
                                             (size_t)(n_ch * ncols) * 4, (size_t)g, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));         // (the class words of this group and the caller's arrays are read until here)
        }
    }
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
