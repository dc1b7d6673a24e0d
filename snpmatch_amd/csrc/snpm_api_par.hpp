// snpm_api_par.hpp -- C ABI: parentsearch -- score / n_tot / w_first / w_het of every pair of accession columns taken per genome window as the parents of a recombinant sample, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- parentsearch
// As snpm_panel_f1_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is checked
// before the panel handle is looked at, so those refusals are reachable without a device.
//
// Slabs: par_plan of snpm_k_par.hpp cuts the windows into slabs of WHOLE windows whose planes fit the workspace budget
// (SNPM_PAR_WS_MB; a window larger than the budget is a slab of its own, the planes workspace grows to it), the slabs into groups of
// whole windows and the groups into masked segments.  The plan of all slabs is made and uploaded once; per slab k_win_planes as it
// stands (`first` = the slab's first selected row) and k_par_count (a launch per 65535 groups) add into the zeroed device matrices,
// so the result does not depend on the budget.  The slab walk is this call's own: its slabs have different lengths.
int snpm_panel_parent_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                             const uint8_t *sample_class, const int64_t *win_off, int64_t n_win, int32_t min_win_sites, int32_t *score,
                             int32_t *n_tot, int32_t *w_first, int32_t *w_het)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, n_win >= 0, "negative number of windows");
    CHECK_ARG(ctx, min_win_sites >= 1, "min_win_sites must be 1 or more");
    CHECK_ARG(ctx, ncols <= SNPM_F1X_MAX_ACCESSIONS, "too many accessions for one call (SNPM_F1X_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: the counts would not fit int32");
    if (int bad = check_offsets(ctx, "win_off", win_off, n_win, n_rows)) return bad;
    if (ncols > 0) CHECK_ARG(ctx, score != nullptr && n_tot != nullptr && w_first != nullptr && w_het != nullptr, "score / n_tot / w_first / w_het is NULL");
    if (n_rows > 0) CHECK_ARG(ctx, sample_class != nullptr, "sample_class is NULL");
    for (int64_t k = 0; k < n_rows; ++k) CHECK_ARG(ctx, sample_class[k] <= 2 || sample_class[k] == 0xFF, "sample_class holds a byte other than 0, 1, 2 or 0xFF");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0) return SNPM_OK;                                  // nothing to write, nothing launched
    const size_t cells = (size_t)ncols * (size_t)ncols;
    int32_t *const outs[4] = {score, n_tot, w_first, w_het};
    const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
    ParPlan plan;                                                    // (lives until the stream is synchronised)
    if (n_rows > 0) par_plan(ctx->par_ws_bytes, cols_pad, sample_class, win_off, n_win, plan);
    if (plan.segs.empty()) {                                         // no row with a class inside a window: zero counts, nothing launched
        for (int32_t *o : outs) memset(o, 0, cells * sizeof(int32_t));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
    const size_t grp_bytes = plan.groups.size() * sizeof(int64_t), off_bytes = plan.step_off.size() * sizeof(int64_t);
    const size_t seg_bytes = plan.segs.size() * sizeof(unsigned long long);
    Scratch sc;                                                      // bit-planes [4][cols_pad][W] of a slab; group table; step offsets; segments; score | n_tot | w_first | w_het; column list; row list
    unsigned long long *d_planes, *d_segs;
    int64_t *d_groups, *d_steps, *d_rows = nullptr;
    int32_t *d_out, *d_cols = nullptr;
    sc.want(d_planes, (size_t)F1X_PLANES * (size_t)cols_pad * (size_t)plan.max_W);
    sc.want(d_groups, plan.groups.size());
    sc.want(d_steps, plan.step_off.size());
    sc.want(d_segs, plan.segs.size());
    sc.want(d_out, 4 * cells);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rows, (size_t)plan.max_rows);
    if ((rc = scratch_commit(ctx, sc))) return rc;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_groups, plan.groups.data(), grp_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_steps, plan.step_off.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_segs, plan.segs.data(), seg_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_out, 0, 4 * cells * sizeof(int32_t), ctx->stream));
    for (const ParSlab &s : plan.slabs) {
        // (stream order: the previous slab's plane kernel has read its rows before this copy lands)
        if (row_idx) HIPCHK(ctx, hipMemcpyAsync(d_rows, row_idx + s.r0, (size_t)s.n_rows * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        {
            ProfScope ps(ctx, PK_WIN_P);
            const dim3 grid((unsigned)s.W, (unsigned)(cols_pad / F1X_PL_COLS));
            hipLaunchKernelGGL(k_win_planes, grid, dim3(WN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               row_idx ? (int64_t)0 : row0 + s.r0, s.n_rows, d_cols, ncols, d_planes, cols_pad, s.W);
            HIPCHK(ctx, hipGetLastError());
        }
        for (int64_t g = s.g_lo; g < s.g_hi; g += PAR_MAX_GRID_Y) {
            ProfScope ps(ctx, PK_PAR_C);
            const dim3 grid((unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)std::min(PAR_MAX_GRID_Y, s.g_hi - g));
            hipLaunchKernelGGL(k_par_count, grid, dim3(PAR_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, s.W,
                               d_groups + g * PAR_GROUP_WORDS, d_steps, d_segs, (int)ncols, n_tiles, (int)min_win_sites, d_out,
                               d_out + cells, d_out + 2 * cells, d_out + 3 * cells);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    for (int k = 0; k < 4; ++k) HIPCHK(ctx, hipMemcpyAsync(outs[k], d_out + (size_t)k * cells, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx and the plan are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
