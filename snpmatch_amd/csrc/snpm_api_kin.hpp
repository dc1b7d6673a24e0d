// snpm_api_kin.hpp -- C ABI: panel kinship -- ninfo / same / diff counts of every pair of accession columns over panel rows, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- kinship
// As snpm_pair_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is checked
// before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row and column
// index lying inside the panel.
int snpm_panel_kinship_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                              int32_t *ninfo, int32_t *same, int32_t *diff)
{
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_KIN_MAX_ACCESSIONS, "too many accessions for one call (SNPM_KIN_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: the counts would not fit int32");
    if (ncols > 0) CHECK_ARG(ctx, ninfo != nullptr && same != nullptr && diff != nullptr, "ninfo / same / diff is NULL");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    } else {
        CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    }
    if (row_idx) {
        for (int64_t r = 0; r < n_rows; ++r) CHECK_ARG(ctx, row_idx[r] >= 0 && row_idx[r] < p->n_snp, "row index outside the panel");
    } else {
        CHECK_ARG(ctx, row0 >= 0 && row0 <= p->n_snp && n_rows <= p->n_snp - row0, "row range outside the panel");
    }
    if (ncols == 0) return SNPM_OK;                                  // nothing to write, nothing launched
    const size_t cells = (size_t)ncols * (size_t)ncols;
    if (n_rows == 0) {                                               // zero counts, nothing launched
        memset(ninfo, 0, cells * sizeof(int32_t));
        memset(same, 0, cells * sizeof(int32_t));
        memset(diff, 0, cells * sizeof(int32_t));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t cols_pad = (ncols + KN_PL_COLS - 1) / KN_PL_COLS * KN_PL_COLS;
    const int n_tiles = (int)((ncols + KN_TILE - 1) / KN_TILE);
    // slabs of the row axis: whole LDS steps (1024 rows) of planes inside the workspace budget -- whole chunks where the budget holds
    // one -- and at most 65535 chunks (grid.y)
    const int64_t step_rows = (int64_t)KN_STEP_WORDS * 64, steps_per_chunk = KN_CHUNK_WORDS / KN_STEP_WORDS;
    const int64_t step_bytes = 3 * cols_pad * KN_STEP_WORDS * 8;
    int64_t slab_steps = std::max<int64_t>(1, (int64_t)(ctx->kin_ws_bytes / (size_t)step_bytes));
    if (slab_steps >= steps_per_chunk) slab_steps = slab_steps / steps_per_chunk * steps_per_chunk;
    slab_steps = std::min<int64_t>(slab_steps, 65535 * steps_per_chunk);
    slab_steps = std::min<int64_t>(slab_steps, (n_rows + step_rows - 1) / step_rows);
    const int64_t slab_rows = slab_steps * step_rows;
    if ((rc = ensure(ctx, ctx->ws_kin_planes, (size_t)slab_steps * (size_t)step_bytes))) return rc;
    if ((rc = ensure(ctx, ctx->ws_kin_out, 3 * cells * sizeof(int32_t)))) return rc;
    if (cols && (rc = ensure(ctx, ctx->ws_kin_cols, (size_t)ncols * sizeof(int32_t)))) return rc;
    if (row_idx && (rc = ensure(ctx, ctx->ws_kin_rows, (size_t)std::min(slab_rows, n_rows) * sizeof(int64_t)))) return rc;   // the rows of ONE slab
    const int32_t *d_cols = cols ? (const int32_t *)ctx->ws_kin_cols.p : nullptr;
    const int64_t *d_rows = row_idx ? (const int64_t *)ctx->ws_kin_rows.p : nullptr;
    int32_t *d_ninfo = (int32_t *)ctx->ws_kin_out.p, *d_same = d_ninfo + cells, *d_diff = d_same + cells;
    unsigned long long *d_planes = (unsigned long long *)ctx->ws_kin_planes.p;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(ctx->ws_kin_cols.p, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_ninfo, 0, 3 * cells * sizeof(int32_t), ctx->stream));
    for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows) {             // the results accumulate on the device across slabs
        const int64_t n_valid = std::min(slab_rows, n_rows - s0);
        const int64_t W = (n_valid + step_rows - 1) / step_rows * KN_STEP_WORDS;      // words per plane row of this slab
        // a row list travels slab by slab (stream order: the previous slab's plane kernel has read its part before this copy lands)
        if (row_idx) HIPCHK(ctx, hipMemcpyAsync(ctx->ws_kin_rows.p, row_idx + s0, (size_t)n_valid * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        {
            ProfScope ps(ctx, PK_KIN_P);
            const dim3 grid((unsigned)W, (unsigned)(cols_pad / KN_PL_COLS));
            hipLaunchKernelGGL(k_kin_planes, grid, dim3(KN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               row_idx ? (int64_t)0 : row0 + s0, n_valid, d_cols, (int)ncols, d_planes, cols_pad, W);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_KIN_C);
            const dim3 grid((unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + KN_CHUNK_WORDS - 1) / KN_CHUNK_WORDS));
            hipLaunchKernelGGL(k_kin_count, grid, dim3(KN_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, W, (int)ncols,
                               n_tiles, d_ninfo, d_same, d_diff);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(ninfo, d_ninfo, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(same, d_same, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(diff, d_diff, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx are read until here)
    return SNPM_OK;
}
