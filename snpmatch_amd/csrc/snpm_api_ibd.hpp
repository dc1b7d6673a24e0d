// snpm_api_ibd.hpp -- C ABI: ibd -- for every pair of accession columns the genome windows in which the two are identical, as counts, runs and two window bitsets, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- ibd
// As snpm_panel_parent_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.
//
// Slabs: ibd_plan of snpm_k_ibd.hpp cuts the windows into slabs of WHOLE windows whose planes fit the workspace budget
// (SNPM_IBD_WS_MB; a window larger than the budget is a slab of its own, the planes workspace grows to it), the slabs into groups of
// whole windows and the groups into masked segments.  The plan of all slabs is made and uploaded once; per slab k_win_planes as it
// stands (`first` = the slab's first selected row) and k_ibd_count (a launch per 65535 groups) add into the zeroed device matrices
// and OR into the zeroed device bitsets, so the result does not depend on the budget; k_ibd_runs reads the bitsets once, after the
// last slab.  The two device bitsets [ncols][ncols][wwords] are needed whether or not the caller wants them back (the runs are made
// from them) and must fit SNPM_IBD_BITS_MB.
int snpm_panel_ibd_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                          const int64_t *win_off, int64_t n_win, int32_t min_win_sites, int32_t max_diff_ppm, int32_t min_run,
                          int32_t *w_used, int32_t *w_shared, int32_t *n_shared, int32_t *d_shared,
                          int32_t *run_max, int32_t *n_runs, int32_t *w_in_runs, uint32_t *used_bits, uint32_t *shared_bits)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, n_win >= 0, "negative number of windows");
    CHECK_ARG(ctx, min_win_sites >= 1, "min_win_sites must be 1 or more");
    CHECK_ARG(ctx, max_diff_ppm >= 0 && max_diff_ppm <= 1000000, "max_diff_ppm must lie in 0 .. 1000000");
    CHECK_ARG(ctx, min_run >= 1, "min_run must be 1 or more");
    CHECK_ARG(ctx, ncols <= SNPM_F1X_MAX_ACCESSIONS, "too many accessions for one call (SNPM_F1X_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: the counts would not fit int32");
    if (int bad = check_offsets(ctx, "win_off", win_off, n_win, n_rows)) return bad;
    int32_t *const outs[7] = {w_used, w_shared, n_shared, d_shared, run_max, n_runs, w_in_runs};
    if (ncols > 0)
        for (int32_t *o : outs) CHECK_ARG(ctx, o != nullptr, "w_used / w_shared / n_shared / d_shared / run_max / n_runs / w_in_runs is NULL");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0) return SNPM_OK;                                  // nothing to write, nothing launched
    const size_t cells = (size_t)ncols * (size_t)ncols;
    const int64_t wwords = (n_win + 31) / 32;
    // (fp64: cells < 2^27 and any n_win, no product can overflow; exact far beyond any budget)
    const double bits_need = 2.0 * (double)cells * (double)wwords * 4.0;
    if (bits_need > (double)ctx->ibd_bits_bytes)
        return set_err(ctx, SNPM_ERR_BADARG, "the two window bitsets of %lld x %lld cells x %lld windows need %.0f bytes on the device, more than SNPM_IBD_BITS_MB allows (%zu bytes): fewer accessions or windows per call, or a larger SNPM_IBD_BITS_MB",
                       (long long)ncols, (long long)ncols, (long long)n_win, bits_need, ctx->ibd_bits_bytes);
    const size_t bit_words = cells * (size_t)wwords;                 // of one bitset
    const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
    IbdPlan plan;                                                    // (lives until the stream is synchronised)
    if (n_rows > 0) ibd_plan(ctx->ibd_ws_bytes, cols_pad, win_off, n_win, plan);
    if (plan.segs.empty()) {                                         // no row inside a window: zero counts, no window used, nothing launched
        for (int32_t *o : outs) memset(o, 0, cells * sizeof(int32_t));
        if (used_bits) memset(used_bits, 0, bit_words * sizeof(uint32_t));
        if (shared_bits) memset(shared_bits, 0, bit_words * sizeof(uint32_t));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
    const size_t grp_bytes = plan.groups.size() * sizeof(int64_t), off_bytes = plan.step_off.size() * sizeof(int64_t);
    const size_t seg_bytes = plan.segs.size() * sizeof(unsigned long long);
    Scratch sc;                                                      // bit-planes [4][cols_pad][W] of a slab; group table; step offsets; segments; the seven matrices; used | shared bitsets; column list; row list
    unsigned long long *d_planes, *d_segs;
    int64_t *d_groups, *d_steps, *d_rows = nullptr;
    int32_t *d_out, *d_cols = nullptr;
    uint32_t *d_ubits;
    sc.want(d_planes, (size_t)F1X_PLANES * (size_t)cols_pad * (size_t)plan.max_W);
    sc.want(d_groups, plan.groups.size());
    sc.want(d_steps, plan.step_off.size());
    sc.want(d_segs, plan.segs.size());
    sc.want(d_out, 7 * cells);
    sc.want(d_ubits, 2 * bit_words);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rows, (size_t)plan.max_rows);
    if ((rc = scratch_commit(ctx, sc))) return rc;
    uint32_t *d_sbits = d_ubits + bit_words;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_groups, plan.groups.data(), grp_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_steps, plan.step_off.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_segs, plan.segs.data(), seg_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_out, 0, 4 * cells * sizeof(int32_t), ctx->stream));       // (k_ibd_runs writes every cell of the other three)
    HIPCHK(ctx, hipMemsetAsync(d_ubits, 0, 2 * bit_words * sizeof(uint32_t), ctx->stream));
    for (const IbdSlab &s : plan.slabs) {
        // (stream order: the previous slab's plane kernel has read its rows before this copy lands)
        if (row_idx) HIPCHK(ctx, hipMemcpyAsync(d_rows, row_idx + s.r0, (size_t)s.n_rows * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        {
            ProfScope ps(ctx, PK_WIN_P);
            const dim3 grid((unsigned)s.W, (unsigned)(cols_pad / F1X_PL_COLS));
            hipLaunchKernelGGL(k_win_planes, grid, dim3(WN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               row_idx ? (int64_t)0 : row0 + s.r0, s.n_rows, d_cols, ncols, d_planes, cols_pad, s.W);
            HIPCHK(ctx, hipGetLastError());
        }
        for (int64_t g = s.g_lo; g < s.g_hi; g += IBD_MAX_GRID_Y) {
            ProfScope ps(ctx, PK_IBD_C);
            const dim3 grid((unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)std::min(IBD_MAX_GRID_Y, s.g_hi - g));
            hipLaunchKernelGGL(k_ibd_count, grid, dim3(IBD_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, s.W,
                               d_groups + g * IBD_GROUP_WORDS, d_steps, d_segs, (int)ncols, n_tiles, (int)min_win_sites, (int)max_diff_ppm, wwords,
                               d_out, d_out + cells, d_out + 2 * cells, d_out + 3 * cells, d_ubits, d_sbits);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    {
        ProfScope ps(ctx, PK_IBD_R);
        const dim3 grid((unsigned)((cells + IBD_RUN_THREADS - 1) / IBD_RUN_THREADS));
        hipLaunchKernelGGL(k_ibd_runs, grid, dim3(IBD_RUN_THREADS), 0, ctx->stream, (const uint32_t *)d_ubits, (const uint32_t *)d_sbits, (int64_t)cells,
                           wwords, (int)min_run, d_out + 4 * cells, d_out + 5 * cells, d_out + 6 * cells);
        HIPCHK(ctx, hipGetLastError());
    }
    for (int k = 0; k < 7; ++k) HIPCHK(ctx, hipMemcpyAsync(outs[k], d_out + (size_t)k * cells, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (used_bits) HIPCHK(ctx, hipMemcpyAsync(used_bits, d_ubits, bit_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (shared_bits) HIPCHK(ctx, hipMemcpyAsync(shared_bits, d_sbits, bit_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx and the plan are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
