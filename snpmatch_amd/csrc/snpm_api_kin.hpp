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
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
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
    // slabs of the row axis: whole LDS steps of planes inside the workspace budget (kin_slab_steps of snpm_k_kin.hpp)
    const int64_t slab_steps = kin_slab_steps(ctx->kin_ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * KN_STEP_ROWS;
    Scratch sc;                                                       // bit-planes [3][cols_pad][W] of a slab; ninfo | same | diff; column list; row list
    unsigned long long *d_planes;
    int32_t *d_ninfo, *d_cols = nullptr;
    int64_t *d_rowlist = nullptr;
    sc.want(d_planes, (size_t)slab_steps * (size_t)kin_step_bytes(cols_pad) / 8);
    sc.want(d_ninfo, 3 * cells);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(slab_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    int32_t *d_same = d_ninfo + cells, *d_diff = d_same + cells;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_ninfo, 0, 3 * cells * sizeof(int32_t), ctx->stream));
    // the results accumulate on the device across slabs
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, slab_rows, [&](const int64_t *d_rows, int64_t first, int64_t, int64_t n_valid) {
        const int64_t W = (n_valid + KN_STEP_ROWS - 1) / KN_STEP_ROWS * KN_STEP_WORDS;      // words per plane row of this slab
        {
            ProfScope ps(ctx, PK_KIN_P);
            const dim3 grid((unsigned)W, (unsigned)(cols_pad / KN_PL_COLS));
            hipLaunchKernelGGL(k_kin_planes, grid, dim3(KN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               first, n_valid, d_cols, (int)ncols, d_planes, cols_pad, W);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_KIN_C);
            const dim3 grid((unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + KN_CHUNK_WORDS - 1) / KN_CHUNK_WORDS));
            hipLaunchKernelGGL(k_kin_count, grid, dim3(KN_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, W, (int)ncols,
                               n_tiles, d_ninfo, d_same, d_diff);
            HIPCHK(ctx, hipGetLastError());
        }
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ninfo, d_ninfo, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(same, d_same, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(diff, d_diff, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx are read until here)
    return SNPM_OK;
}
