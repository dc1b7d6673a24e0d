// snpm_api_pca.hpp -- C ABI: pca -- the weighted Gram matrix of the accession columns over panel rows and the row-streaming product for the SNP loadings, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- pca
// As snpm_panel_kinship_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row and
// column index lying inside the panel and on every table and vector entry being finite: a NaN must never meet the 0 of a missing call.
//
// Slabs of snpm_panel_gram: pca_slab_steps of snpm_k_pca.hpp cuts the row axis so that the planes and the table rows of a slab fit the
// workspace budget (SNPM_PCA_WS_MB).  Three launches per slab -- k_win_planes as it stands, k_pca_gram into the partials of its
// blocks, k_pca_fold from the partials into the matrix -- so the matrix accumulates on the device across slabs, in slab order.  The
// partials ([splits][tile pairs][64][64] fp64) and the matrix itself are results, not part of the budget.
namespace {
bool pca_all_finite(const double *v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}
}  // namespace

int snpm_panel_gram(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                    const double *tab, double *gram)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_PCA_MAX_ACCESSIONS, "too many accessions for one call (SNPM_PCA_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more");
    if (ncols > 0) CHECK_ARG(ctx, gram != nullptr, "gram is NULL");
    if (ncols > 0 && n_rows > 0) CHECK_ARG(ctx, tab != nullptr, "tab is NULL");
    if (tab) CHECK_ARG(ctx, pca_all_finite(tab, (size_t)n_rows * 4), "tab holds a value that is not finite");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0) return SNPM_OK;                                  // nothing to write, nothing launched
    const size_t cells = (size_t)ncols * (size_t)ncols;
    if (n_rows == 0) {                                               // a zero matrix, nothing launched
        memset(gram, 0, cells * sizeof(double));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t cols_pad = (ncols + PCA_PL_COLS - 1) / PCA_PL_COLS * PCA_PL_COLS;
    const int n_tiles = (int)(cols_pad / PCA_TILE), n_pairs = n_tiles * (n_tiles + 1) / 2, splits = pca_gram_splits(n_pairs);
    const int64_t slab_steps = pca_slab_steps(ctx->pca_ws_bytes, cols_pad, n_rows), slab_rows = slab_steps * PCA_STEP_ROWS;
    const size_t plane_bytes = (size_t)slab_steps * (size_t)(4 * cols_pad * PCA_STEP_WORDS * 8);
    Scratch sc;                                                      // bit-planes [4][cols_pad][W] and table rows of a slab; partials [splits][tile pairs][64][64]; the matrix; column list; row list
    unsigned long long *d_planes;
    double *d_tab, *d_part, *d_gram;
    int32_t *d_cols = nullptr;
    int64_t *d_rowlist = nullptr;
    sc.want(d_planes, plane_bytes / 8);
    sc.want(d_tab, (size_t)std::min(slab_rows, n_rows) * 4);
    sc.want(d_part, (size_t)splits * (size_t)n_pairs * PCA_TILE * PCA_TILE);
    sc.want(d_gram, cells);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(slab_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_gram, 0, cells * sizeof(double), ctx->stream));
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, slab_rows, [&](const int64_t *d_rows, int64_t first, int64_t s0, int64_t n_valid) {
        const int64_t W = (n_valid + PCA_STEP_ROWS - 1) / PCA_STEP_ROWS * PCA_STEP_WORDS;    // words per plane row of this slab
        // (stream order: the previous slab's k_pca_gram has read its table rows before this copy lands)
        HIPCHK(ctx, hipMemcpyAsync(d_tab, tab + 4 * s0, (size_t)n_valid * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        {
            ProfScope ps(ctx, PK_WIN_P);
            const dim3 grid((unsigned)W, (unsigned)(cols_pad / PCA_PL_COLS));
            hipLaunchKernelGGL(k_win_planes, grid, dim3(WN_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows,
                               first, n_valid, d_cols, ncols, d_planes, cols_pad, W);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_PCA_G);
            hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)n_pairs, (unsigned)splits), dim3(PCA_THREADS), 0, ctx->stream,
                               (const unsigned long long *)d_planes, cols_pad, W, (const double *)d_tab, n_valid, n_tiles, d_part);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_PCA_F);
            hipLaunchKernelGGL(k_pca_fold, dim3((unsigned)((cells + PCA_THREADS - 1) / PCA_THREADS)), dim3(PCA_THREADS), 0, ctx->stream,
                               (const double *)d_part, n_tiles, n_pairs, splits, ncols, d_gram);
            HIPCHK(ctx, hipGetLastError());
        }
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(gram, d_gram, cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx / tab are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))

// Slabs of snpm_panel_loadings: pca_load_slab_rows rows whose table rows, results and list entries fit the same budget; one launch
// per slab, its results are copied to the caller's array in stream order before the next slab's launch overwrites them.
int snpm_panel_loadings(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                        const double *tab, const double *vec, int k, double *load)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_PCA_MAX_ACCESSIONS, "too many accessions for one call (SNPM_PCA_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, k >= 1 && k <= SNPM_PCA_MAX_COMPONENTS, "k outside 1 .. SNPM_PCA_MAX_COMPONENTS");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more");
    if (ncols > 0) CHECK_ARG(ctx, vec != nullptr, "vec is NULL");
    if (ncols > 0 && n_rows > 0) CHECK_ARG(ctx, tab != nullptr && load != nullptr, "tab / load is NULL");
    if (tab) CHECK_ARG(ctx, pca_all_finite(tab, (size_t)n_rows * 4), "tab holds a value that is not finite");
    if (vec) CHECK_ARG(ctx, pca_all_finite(vec, (size_t)ncols * (size_t)k), "vec holds a value that is not finite");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0 || n_rows == 0) return SNPM_OK;                   // nothing to write, nothing launched
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t slab_rows = pca_load_slab_rows(ctx->pca_ws_bytes, k, n_rows);
    const int kp = pca_load_pitch(k);                                // vec rows padded with zeros to whole groups of components
    Scratch sc;                                                      // table rows and loadings of a slab; vec [ncols][kp]; column list; row list
    double *d_tab, *d_load, *d_vec;
    int32_t *d_cols = nullptr;
    int64_t *d_rowlist = nullptr;
    sc.want(d_tab, (size_t)slab_rows * 4);
    sc.want(d_load, (size_t)slab_rows * (size_t)k);
    sc.want(d_vec, (size_t)ncols * (size_t)kp);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(slab_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (kp != k) HIPCHK(ctx, hipMemsetAsync(d_vec, 0, (size_t)ncols * (size_t)kp * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemcpy2DAsync(d_vec, (size_t)kp * sizeof(double), vec, (size_t)k * sizeof(double), (size_t)k * sizeof(double), (size_t)ncols,
                                 hipMemcpyHostToDevice, ctx->stream));
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, slab_rows, [&](const int64_t *d_rows, int64_t first, int64_t s0, int64_t n_valid) {
        HIPCHK(ctx, hipMemcpyAsync(d_tab, tab + 4 * s0, (size_t)n_valid * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        {
            ProfScope ps(ctx, PK_PCA_L);
            constexpr int waves = PCA_LOAD_THREADS / WAVE;
            const int64_t blocks = std::min<int64_t>((n_valid + waves - 1) / waves, (int64_t)ctx->n_cu * 16);
            hipLaunchKernelGGL(k_pca_load, dim3((unsigned)blocks), dim3(PCA_LOAD_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch,
                               p->desc, d_rows, first, n_valid, d_cols, ncols, (const double *)d_tab, (const double *)d_vec, k, d_load);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipMemcpyAsync(load + s0 * k, d_load, (size_t)n_valid * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx / tab / vec are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
