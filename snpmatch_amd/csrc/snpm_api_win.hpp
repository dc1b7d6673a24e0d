// snpm_api_win.hpp -- C ABI: panel windows -- per genome window the call counts of every listed accession column and the agreement counts of listed pairs of columns, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- panel windows
// As snpm_panel_kinship_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row,
// column and pair index lying inside its range and on win_off being a sound offset table over the selected rows.
//
// Slabs: win_slab_steps of snpm_k_win.hpp walks win_off and cuts the selected rows so that the planes and the cells of a slab fit
// the workspace budget (SNPM_WIN_WS_MB).  Two launches per slab write the cells of the slab's contiguous window range into a
// workspace; the workspace is copied to the host and ADDED into the caller's zeroed arrays, so a window that spans slabs is summed
// there and the result does not depend on the budget.
int snpm_panel_window_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs,
                             const int64_t *row_idx, int64_t row0, int64_t n_rows, const int64_t *win_off, int64_t n_win, int32_t *acc_counts,
                             int32_t *pair_counts)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_pairs >= 0 && n_rows >= 0 && n_win >= 0, "negative size");
    if (int bad = check_offsets(ctx, "win_off", win_off, n_win, n_rows)) return bad;
    if (n_win > 0 && ncols > 0) CHECK_ARG(ctx, acc_counts != nullptr || pair_counts != nullptr, "acc_counts and pair_counts are both NULL");
    if (n_pairs > 0) CHECK_ARG(ctx, pair_a != nullptr && pair_b != nullptr, "pair_a / pair_b is NULL");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: the counts would not fit int32");
    CHECK_ARG(ctx, ncols <= SNPM_WIN_MAX_ACCESSIONS, "too many accessions for one call (SNPM_WIN_MAX_ACCESSIONS)");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    } else {
        CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    }
    for (int64_t i = 0; i < n_pairs; ++i)
        CHECK_ARG(ctx, pair_a[i] >= 0 && pair_a[i] < ncols && pair_b[i] >= 0 && pair_b[i] < ncols, "pair index outside the column list");
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (n_win == 0 || ncols == 0) return SNPM_OK;                    // nothing to write, nothing launched
    const int64_t acc_cols = acc_counts ? ncols : 0, pairs = pair_counts ? n_pairs : 0;
    if (acc_counts) memset(acc_counts, 0, (size_t)n_win * (size_t)ncols * 4 * sizeof(int32_t));
    if (pairs) memset(pair_counts, 0, (size_t)pairs * (size_t)n_win * 4 * sizeof(int32_t));
    if (n_rows == 0 || acc_cols + pairs == 0) return SNPM_OK;       // zero counts, nothing launched
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t cols_pad = (ncols + WN_PL_COLS - 1) / WN_PL_COLS * WN_PL_COLS, cell_bytes = 16 * (acc_cols + pairs);
    // the plan: every slab, then the workspaces by the largest
    struct Slab { int64_t s0, steps, w_lo, n_w; };
    std::vector<Slab> slabs;
    int64_t max_steps = 0, max_w = 0, max_rows = 0;
    for (int64_t s0 = 0, w_lo = 0, w_end = 0; s0 < n_rows;) {
        const int64_t steps = win_slab_steps(ctx->win_ws_bytes, cols_pad, cell_bytes, win_off, n_win, n_rows, s0, w_lo, w_end);
        slabs.push_back({s0, steps, w_lo, w_end - w_lo});
        max_steps = std::max(max_steps, steps);
        max_w = std::max(max_w, w_end - w_lo);
        max_rows = std::max(max_rows, std::min(steps * WN_STEP_ROWS, n_rows - s0));
        s0 += steps * WN_STEP_ROWS;
    }
    Scratch sc;                                                      // bit-planes [4][cols_pad][W] and cells of a slab; win_off; column list; pa | pb; row list
    unsigned long long *d_planes;
    int32_t *d_cells, *d_cols = nullptr, *d_pa = nullptr;
    int64_t *d_off, *d_rows = nullptr;
    sc.want(d_planes, (size_t)max_steps * (size_t)win_step_bytes(cols_pad) / 8);
    sc.want(d_cells, (size_t)max_w * (size_t)cell_bytes / 4);
    sc.want(d_off, (size_t)(n_win + 1));
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (pairs) sc.want(d_pa, 2 * (size_t)pairs);
    if (row_idx) sc.want(d_rows, (size_t)max_rows);
    if ((rc = scratch_commit(ctx, sc))) return rc;
    int32_t *d_pb = pairs ? d_pa + pairs : nullptr;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (pairs) {
        HIPCHK(ctx, hipMemcpyAsync(d_pa, pair_a, (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_pb, pair_b, (size_t)pairs * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(d_off, win_off, (size_t)(n_win + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    std::vector<int32_t> host_cells((size_t)max_w * (size_t)(acc_cols + pairs) * 4);
    for (const Slab &sl : slabs) {
        const int64_t n_valid = std::min(sl.steps * WN_STEP_ROWS, n_rows - sl.s0);
        const int64_t W = (n_valid + WN_STEP_ROWS - 1) / WN_STEP_ROWS * WN_STEP_WORDS;     // words per plane row of this slab
        // (a row list travels slab by slab; the previous slab's stream was synchronised, so its rows are no longer read)
        if (row_idx) HIPCHK(ctx, hipMemcpyAsync(d_rows, row_idx + sl.s0, (size_t)n_valid * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        {
            ProfScope ps(ctx, PK_WIN_P);
            const dim3 grid((unsigned)W, (unsigned)(cols_pad / WN_PL_COLS));
            hipLaunchKernelGGL(k_win_planes, grid, dim3(WN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               row_idx ? (int64_t)0 : row0 + sl.s0, n_valid, d_cols, ncols, d_planes, cols_pad, W);
            HIPCHK(ctx, hipGetLastError());
        }
        const int64_t items = sl.n_w * (acc_cols + pairs);
        {
            ProfScope ps(ctx, PK_WIN_C);
            const int lg = win_group_lg(n_valid, sl.n_w);
            const int64_t per_block = WN_THREADS >> lg, blocks = (items + per_block - 1) / per_block;
            const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)ctx->n_cu * 64)));
            hipLaunchKernelGGL(k_win_count, grid, dim3(WN_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, W, sl.s0, n_valid,
                               (const int64_t *)d_off, sl.w_lo, sl.n_w, acc_cols, d_pa, d_pb, pairs, lg, d_cells);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipMemcpyAsync(host_cells.data(), d_cells, (size_t)items * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        // the slab's cells into the caller's arrays: [n_w][ncols][4] is a contiguous run of acc_counts; [pairs][n_w][4] one run per pair
        const int32_t *src = host_cells.data();
        if (acc_cols) {
            int32_t *dst = acc_counts + sl.w_lo * ncols * 4;
            for (int64_t k = 0; k < sl.n_w * ncols * 4; ++k) dst[k] += src[k];
            src += sl.n_w * ncols * 4;
        }
        for (int64_t i = 0; i < pairs; ++i) {
            int32_t *dst = pair_counts + (i * n_win + sl.w_lo) * 4;
            for (int64_t k = 0; k < sl.n_w * 4; ++k) dst[k] += src[i * sl.n_w * 4 + k];
        }
    }
    return SNPM_OK;                                                  // (the stream is synchronised: the caller's lists are no longer read)
} SNPM_GUARD((panel ? panel->ctx : nullptr))
