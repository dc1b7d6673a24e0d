// snpm_api_sim.hpp -- C ABI: power -- score / ninfo of the sample simulated from every accession column against every accession column, per group of selected rows, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- power
// As snpm_panel_f1_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row and
// column index lying inside the panel and on a sound grp_off.
//
// Slabs: sim_slab_steps of snpm_k_sim.hpp cuts the row axis so that the SEVEN planes of a slab (P0, P1, P2, I of k_win_planes and the
// sample planes Q0, Q1, Q2 of k_sim_noise) fit the workspace budget (SNPM_SIM_WS_MB).  Three launches per slab -- k_win_planes as it
// stands, k_sim_noise (not with err_thr == 0), k_sim_count -- add into the zeroed device arrays, so the result does not depend on the
// budget: the hash is keyed by the position of a row in the selection, not by its place in a slab.
int snpm_panel_sim_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                          const int64_t *grp_off, int64_t n_grp, uint64_t err_thr, uint64_t seed, int32_t *score, int32_t *ninfo)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_SIM_MAX_ACCESSIONS, "too many accessions for one call (SNPM_SIM_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: the counts would not fit int32");
    CHECK_ARG(ctx, n_grp >= 1 && n_grp <= SIM_MAX_GROUPS, "n_grp must be 1 .. 64");
    CHECK_ARG(ctx, n_grp * ncols * ncols <= INT32_MAX, "n_grp * ncols * ncols must stay below 2^31 cells");
    if (int bad = check_offsets(ctx, "grp_off", grp_off, n_grp, n_rows)) return bad;
    CHECK_ARG(ctx, err_thr <= (uint64_t)1 << 32, "err_thr must be 0 .. 2^32");
    if (ncols > 0) CHECK_ARG(ctx, score != nullptr && ninfo != nullptr, "score / ninfo is NULL");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0) return SNPM_OK;                                  // nothing to write, nothing launched
    const size_t cells = (size_t)n_grp * (size_t)ncols * (size_t)ncols;
    if (n_rows == 0) {                                               // zero counts, nothing launched
        memset(score, 0, cells * sizeof(int32_t));
        memset(ninfo, 0, cells * sizeof(int32_t));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t cols_pad = (ncols + F1X_PL_COLS - 1) / F1X_PL_COLS * F1X_PL_COLS;
    const int n_tiles = (int)((ncols + F1X_TILE - 1) / F1X_TILE);
    const bool noisy = err_thr != 0;
    // slabs of the row axis: whole LDS steps of the seven planes inside the workspace budget (sim_slab_steps of snpm_k_sim.hpp)
    const int64_t slab_steps = sim_slab_steps(ctx->sim_ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * F1X_STEP_ROWS;
    const size_t slab_plane_words = (size_t)cols_pad * (size_t)slab_steps * F1X_STEP_WORDS;      // words of one plane of a full slab
    Scratch sc;                                                      // bit-planes [4 + 3][cols_pad][W] of a slab; grp_off; score | ninfo; column list; row list
    unsigned long long *d_planes;
    int64_t *d_grp, *d_rowlist = nullptr;
    int32_t *d_score, *d_cols = nullptr;
    sc.want(d_planes, (size_t)slab_steps * (size_t)sim_step_bytes(cols_pad) / 8);
    sc.want(d_grp, (size_t)(n_grp + 1));
    sc.want(d_score, 2 * cells);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(slab_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    int32_t *d_ninfo = d_score + cells;
    unsigned long long *d_q = d_planes + F1X_PLANES * slab_plane_words;          // (behind the P planes of the LARGEST slab)
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_grp, grp_off, (size_t)(n_grp + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_score, 0, 2 * cells * sizeof(int32_t), ctx->stream));
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
        if (noisy) {
            ProfScope ps(ctx, PK_SIM_N);
            const dim3 grid((unsigned)((W + WAVE - 1) / WAVE), (unsigned)(cols_pad / (SIM_THREADS / WAVE)));
            hipLaunchKernelGGL(k_sim_noise, grid, dim3(SIM_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes, d_q, cols_pad, W, s0,
                               (unsigned long long)err_thr, (unsigned long long)seed);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_SIM_C);
            const dim3 grid((unsigned)(n_tiles * n_tiles), (unsigned)((W + F1X_CHUNK_WORDS - 1) / F1X_CHUNK_WORDS));
            hipLaunchKernelGGL(k_sim_count, grid, dim3(SIM_THREADS), 0, ctx->stream, (const unsigned long long *)d_planes,
                               (const unsigned long long *)(noisy ? d_q : d_planes), cols_pad, W, s0, d_grp, (int)n_grp, (int)ncols, n_tiles,
                               d_score, d_ninfo);
            HIPCHK(ctx, hipGetLastError());
        }
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(score, d_score, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ninfo, d_ninfo, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx / grp_off are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
