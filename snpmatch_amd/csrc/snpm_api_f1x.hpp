// snpm_api_f1x.hpp -- C ABI: f1search -- hits / ninfo of the in-silico F1 of every pair of accession columns against one sample's hard calls over panel rows, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- f1search
// As snpm_panel_kinship_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row and
// column index lying inside the panel; a class byte outside 0 / 1 / 2 / 0xFF is refused rather than read as "no class".
//
// Slabs: f1x_slab_steps of snpm_k_f1x.hpp cuts the row axis so that the planes of a slab fit the workspace budget (SNPM_F1X_WS_MB).
// Two launches per slab -- k_win_planes as it stands, then k_f1x_count -- add into the zeroed device matrices, so the result does not
// depend on the budget.  The sample's masks (3 bits per row) are made on the host for all rows and uploaded once.
int snpm_panel_f1_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                         const uint8_t *sample_class, int32_t *hits, int32_t *ninfo)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_F1X_MAX_ACCESSIONS, "too many accessions for one call (SNPM_F1X_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: the counts would not fit int32");
    if (ncols > 0) CHECK_ARG(ctx, hits != nullptr && ninfo != nullptr, "hits / ninfo is NULL");
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
    if (n_rows == 0) {                                               // zero counts, nothing launched
        memset(hits, 0, cells * sizeof(int32_t));
        memset(ninfo, 0, cells * sizeof(int32_t));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
    const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
    // slabs of the row axis: whole LDS steps of planes inside the workspace budget (f1x_slab_steps of snpm_k_f1x.hpp)
    const int64_t slab_steps = f1x_slab_steps(ctx->f1x_ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * F1X_STEP_ROWS;
    const int64_t all_steps = (n_rows + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS;
    std::vector<unsigned long long> masks((size_t)all_steps * F1X_MASK_WORDS);      // (lives until the stream is synchronised)
    f1x_fill_masks(sample_class, n_rows, masks.data());
    Scratch sc;                                                      // bit-planes [4][cols_pad][W] of a slab; sample masks of all rows; hits | ninfo; column list; row list
    unsigned long long *d_planes, *d_masks;
    int32_t *d_hits, *d_cols = nullptr;
    int64_t *d_rowlist = nullptr;
    sc.want(d_planes, (size_t)slab_steps * (size_t)f1x_step_bytes(cols_pad) / 8);
    sc.want(d_masks, masks.size());
    sc.want(d_hits, 2 * cells);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(slab_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    int32_t *d_ninfo = d_hits + cells;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_masks, masks.data(), masks.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_hits, 0, 2 * cells * sizeof(int32_t), ctx->stream));
    // the results accumulate on the device across slabs
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, slab_rows, [&](const int64_t *d_rows, int64_t first, int64_t s0, int64_t n_valid) {
        const int64_t W = (n_valid + F1X_STEP_ROWS - 1) / F1X_STEP_ROWS * F1X_STEP_WORDS;    // words per plane row of this slab
        {
            ProfScope ps(ctx, PK_WIN_P);
            const dim3 grid((unsigned)W, (unsigned)(cols_pad / F1X_PL_COLS));
            hipLaunchKernelGGL(k_win_planes, grid, dim3(WN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               first, n_valid, d_cols, ncols, d_planes, cols_pad, W);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_F1X_C);
            const dim3 grid((unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + F1X_CHUNK_WORDS - 1) / F1X_CHUNK_WORDS));
            hipLaunchKernelGGL(k_f1x_count, grid, dim3(F1X_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, W,
                               d_masks + s0 / F1X_STEP_ROWS * F1X_MASK_WORDS, (int)ncols, n_tiles, d_hits, d_ninfo);
            HIPCHK(ctx, hipGetLastError());
        }
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(hits, d_hits, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ninfo, d_ninfo, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx and the masks are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
