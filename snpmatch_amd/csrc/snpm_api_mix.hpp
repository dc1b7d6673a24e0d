// snpm_api_mix.hpp -- C ABI: mixture -- the read-count-weighted 2 x 2 tables of every ordered pair of accession columns against one sample's allele depths over panel rows, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- mixture
// As snpm_panel_f1_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row and
// column index lying inside the panel.
//
// Slabs: mix_slab_steps of snpm_k_mix.hpp cuts the row axis so that the planes of a slab fit the workspace budget (SNPM_MIX_WS_MB).
// Two launches per slab -- k_win_planes as it stands, then k_mix_count<BITS> with the smallest BITS of 2 / 4 / 8 that holds the
// largest count of the call -- add into the zeroed device table, so the result does not depend on the budget.  The sample's bit
// slices (2 BITS bits per row) are made on the host for all rows and uploaded once.
int snpm_panel_mix_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                          const uint8_t *alt, const uint8_t *ref, int32_t *table)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_MIX_MAX_ACCESSIONS, "too many accessions for one call (SNPM_MIX_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: the sums would not fit int32");
    if (ncols > 0) CHECK_ARG(ctx, table != nullptr, "table is NULL");
    if (n_rows > 0) CHECK_ARG(ctx, alt != nullptr && ref != nullptr, "alt / ref is NULL");
    int max_count = 0;
    for (int64_t k = 0; k < n_rows; ++k) max_count = std::max(max_count, (int)std::max(alt[k], ref[k]));
    CHECK_ARG(ctx, n_rows * (int64_t)max_count <= (int64_t)INT32_MAX, "n_rows * the largest read count reaches 2^31: the sums would not fit int32");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0) return SNPM_OK;                                  // nothing to write, nothing launched
    const size_t cells = (size_t)ncols * (size_t)ncols;
    if (n_rows == 0) {                                               // zero sums, nothing launched
        memset(table, 0, 8 * cells * sizeof(int32_t));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int bits = mix_bits_of(max_count);
    const int64_t mask_words = mix_mask_words(bits);
    const int64_t cols_pad = (ncols + MIX_PL_COLS - 1) / MIX_PL_COLS * MIX_PL_COLS;
    const int n_tiles = (int)((ncols + MIX_TILE - 1) / MIX_TILE);
    // slabs of the row axis: whole LDS steps of planes inside the workspace budget (mix_slab_steps of snpm_k_mix.hpp)
    const int64_t slab_steps = mix_slab_steps(ctx->mix_ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * MIX_STEP_ROWS;
    const int64_t all_steps = (n_rows + MIX_STEP_ROWS - 1) / MIX_STEP_ROWS;
    std::vector<unsigned long long> masks((size_t)(all_steps * mask_words));        // (lives until the stream is synchronised)
    mix_fill_masks(alt, ref, n_rows, bits, masks.data());
    Scratch sc;                                                      // bit-planes [4][cols_pad][W] of a slab; bit slices of the read counts of all rows; the table [2][2][2][ncols][ncols]; column list; row list
    unsigned long long *d_planes, *d_masks;
    int32_t *d_out, *d_cols = nullptr;
    int64_t *d_rowlist = nullptr;
    sc.want(d_planes, (size_t)slab_steps * (size_t)mix_step_bytes(cols_pad) / 8);
    sc.want(d_masks, masks.size());
    sc.want(d_out, 8 * cells);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(slab_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_masks, masks.data(), masks.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_out, 0, 8 * cells * sizeof(int32_t), ctx->stream));
    // the sums accumulate on the device across slabs
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, slab_rows, [&](const int64_t *d_rows, int64_t first, int64_t s0, int64_t n_valid) {
        const int64_t W = (n_valid + MIX_STEP_ROWS - 1) / MIX_STEP_ROWS * MIX_STEP_WORDS;    // words per plane row of this slab
        {
            ProfScope ps(ctx, PK_WIN_P);
            const dim3 grid((unsigned)W, (unsigned)(cols_pad / MIX_PL_COLS));
            hipLaunchKernelGGL(k_win_planes, grid, dim3(WN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               first, n_valid, d_cols, ncols, d_planes, cols_pad, W);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_MIX_C);
            const dim3 grid((unsigned)(n_tiles * (n_tiles + 1) / 2), (unsigned)((W + MIX_CHUNK_WORDS - 1) / MIX_CHUNK_WORDS));
            const unsigned long long *slab_masks = d_masks + s0 / MIX_STEP_ROWS * mask_words;
            if (bits == 2)
                hipLaunchKernelGGL(k_mix_count<2>, grid, dim3(MIX_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, W,
                                   slab_masks, (int)ncols, n_tiles, d_out);
            else if (bits == 4)
                hipLaunchKernelGGL(k_mix_count<4>, grid, dim3(MIX_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, W,
                                   slab_masks, (int)ncols, n_tiles, d_out);
            else
                hipLaunchKernelGGL(k_mix_count<8>, grid, dim3(MIX_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, cols_pad, W,
                                   slab_masks, (int)ncols, n_tiles, d_out);
            HIPCHK(ctx, hipGetLastError());
        }
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(table, d_out, 8 * cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx and the masks are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
