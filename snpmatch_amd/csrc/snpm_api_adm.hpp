// snpm_api_adm.hpp -- C ABI: admixture -- joint EM iterations of the admixture model on the accession columns of the resident panel, the parameters on the device between iterations (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- admixture
// As snpm_panel_gram: everything is validated on the host BEFORE the device is touched; what does not need the panel is checked
// before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row and column
// index lying inside the panel, on the rows of Q being non-negative and summing to 1 and on F lying inside [EPS, 1 - EPS]: then p
// and pbar of every cell are at least EPS and no division by zero can occur.
//
// No slabs and no workspace knob: the panel is resident, the row list (8 bytes per row) travels once, Q and F are copied in once
// into rows of adm_pitch(K) doubles, double-buffered -- an iteration reads one pair and writes the other, a component that is not
// updated is not swapped -- and are copied out once; scratch_commit reports what does not fit.  Per iteration k_adm_rows (F', the likelihood
// per block of rows), with SNPM_ADMIX_UPDATE_Q k_adm_cols (the partials of its splits), and k_adm_fold (Q', the likelihood).
extern "C++" {                              // (a template cannot have C linkage)
namespace {
template <int KT>
void adm_launch(snpm_ctx *ctx, const snpm_panel *p, const int64_t *d_rows, int64_t first, int64_t n_rows, const int32_t *d_cols, int64_t ncols, int K,
                unsigned flags, const double *q_old, double *q_new, const double *f_old, double *f_new, double *d_part, double *d_ll, double *d_out)
{
    const int64_t n_ll = adm_ll_blocks(n_rows), splits = adm_splits(n_rows, ncols);
    const bool up_q = (flags & SNPM_ADMIX_UPDATE_Q) != 0;
    {
        ProfScope ps(ctx, PK_ADM_R);
        hipLaunchKernelGGL(k_adm_rows<KT>, dim3((unsigned)n_ll), dim3(ADM_ROWS_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc,
                           d_rows, first, n_rows, d_cols, ncols, q_old, f_old, K, (int)(flags & SNPM_ADMIX_UPDATE_F), f_new, d_ll);
    }
    if (up_q) {
        ProfScope ps(ctx, PK_ADM_C);
        const dim3 grid((unsigned)((ncols + ADM_COLS_THREADS - 1) / ADM_COLS_THREADS), (unsigned)splits);
        hipLaunchKernelGGL(k_adm_cols<KT>, grid, dim3(ADM_COLS_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, d_rows, first,
                           n_rows, adm_split_rows(n_rows, ncols), d_cols, ncols, q_old, f_old, d_part);
    }
    {
        ProfScope ps(ctx, PK_ADM_F);
        const unsigned col_blocks = up_q ? (unsigned)adm_fold_col_blocks(ncols, KT) : 0u;
        hipLaunchKernelGGL(k_adm_fold<KT>, dim3(col_blocks + 1), dim3(ADM_FOLD_THREADS), 0, ctx->stream, (const double *)d_part, splits, ncols, q_old,
                           q_new, d_ll, d_ll + n_ll, n_ll, d_out);
    }
}
}  // namespace
}  // extern "C++"

int snpm_panel_admix(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows, int K,
                     int n_iter, unsigned flags, double *Q, double *F, double *loglik)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, ncols <= SNPM_PCA_MAX_ACCESSIONS, "too many accessions for one call (SNPM_PCA_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more");
    CHECK_ARG(ctx, K >= 1 && K <= SNPM_ADMIX_MAX_K, "K outside 1 .. SNPM_ADMIX_MAX_K");
    CHECK_ARG(ctx, n_iter >= 1 && n_iter <= 10000, "n_iter outside 1 .. 10000");
    CHECK_ARG(ctx, (flags & ~(unsigned)(SNPM_ADMIX_UPDATE_F | SNPM_ADMIX_UPDATE_Q)) == 0, "unknown flag bits (SNPM_ADMIX_UPDATE_F | SNPM_ADMIX_UPDATE_Q)");
    if (ncols > 0) CHECK_ARG(ctx, Q != nullptr && loglik != nullptr, "Q / loglik is NULL");
    if (ncols > 0 && n_rows > 0) CHECK_ARG(ctx, F != nullptr, "F is NULL");
    if (Q) {
        for (int64_t i = 0; i < ncols; ++i) {
            double sum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double q = Q[i * K + k];
                CHECK_ARG(ctx, std::isfinite(q) && q >= 0.0, "Q holds an entry that is not finite or is negative");
                sum += q;
            }
            CHECK_ARG(ctx, std::fabs(sum - 1.0) <= 1e-9, "a row of Q does not sum to 1 (within 1e-9)");
        }
    }
    if (F) {
        for (int64_t i = 0; i < n_rows * K; ++i)
            CHECK_ARG(ctx, F[i] >= SNPM_ADMIX_EPS && F[i] <= 1.0 - SNPM_ADMIX_EPS, "F holds an entry outside [SNPM_ADMIX_EPS, 1 - SNPM_ADMIX_EPS]");
    }
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    if (!cols) CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    if (ncols == 0) return SNPM_OK;                                  // nothing to write, nothing launched
    if (n_rows == 0) {                                               // no cell: likelihood 0, nothing launched
        memset(loglik, 0, (size_t)n_iter * sizeof(double));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int kt = adm_pitch(K);
    const size_t q_doubles = (size_t)ncols * (size_t)kt, f_doubles = (size_t)n_rows * (size_t)kt;
    const int64_t n_ll = adm_ll_blocks(n_rows), splits = adm_splits(n_rows, ncols);
    Scratch sc;     // Q and Q' [2][ncols][KT]; F and F' [2][n_rows][KT]; partials [splits][ncols][KT]; the two buffers of the likelihood tree; loglik [n_iter]; column list; row list
    double *d_qq, *d_ff, *d_part, *d_ll, *d_out;
    int32_t *d_cols = nullptr;
    int64_t *d_rowlist = nullptr;
    sc.want(d_qq, 2 * q_doubles);
    sc.want(d_ff, 2 * f_doubles);
    sc.want(d_part, (size_t)splits * q_doubles);
    sc.want(d_ll, (size_t)(n_ll + (n_ll + ADM_TREE_RADIX - 1) / ADM_TREE_RADIX));
    sc.want(d_out, (size_t)n_iter);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rowlist, (size_t)n_rows);
    if ((rc = scratch_commit(ctx, sc))) return rc;
    double *d_q[2] = {d_qq, d_qq + q_doubles}, *d_f[2] = {d_ff, d_ff + f_doubles};
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    // rows of kt doubles, the entries at and beyond K zero, in both copies: k_adm_rows never writes them
    std::vector<double> hq(q_doubles, 0.0), hf(f_doubles, 0.0);
    for (int64_t i = 0; i < ncols; ++i) memcpy(&hq[(size_t)i * kt], Q + i * K, (size_t)K * sizeof(double));
    for (int64_t s = 0; s < n_rows; ++s) memcpy(&hf[(size_t)s * kt], F + s * K, (size_t)K * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(d_q[0], hq.data(), q_doubles * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_f[0], hf.data(), f_doubles * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_q[1], 0, q_doubles * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_f[1], 0, f_doubles * sizeof(double), ctx->stream));
    int at_q = 0, at_f = 0;
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, n_rows, [&](const int64_t *d_rows, int64_t first, int64_t, int64_t) {      // (one slab: all rows)
        for (int t = 0; t < n_iter; ++t) {
            switch (kt) {
            case 4: adm_launch<4>(ctx, p, d_rows, first, n_rows, d_cols, ncols, K, flags, d_q[at_q], d_q[at_q ^ 1], d_f[at_f], d_f[at_f ^ 1], d_part, d_ll, d_out + t); break;
            case 8: adm_launch<8>(ctx, p, d_rows, first, n_rows, d_cols, ncols, K, flags, d_q[at_q], d_q[at_q ^ 1], d_f[at_f], d_f[at_f ^ 1], d_part, d_ll, d_out + t); break;
            default: adm_launch<16>(ctx, p, d_rows, first, n_rows, d_cols, ncols, K, flags, d_q[at_q], d_q[at_q ^ 1], d_f[at_f], d_f[at_f ^ 1], d_part, d_ll, d_out + t); break;
            }
            HIPCHK(ctx, hipGetLastError());
            if (flags & SNPM_ADMIX_UPDATE_Q) at_q ^= 1;
            if (flags & SNPM_ADMIX_UPDATE_F) at_f ^= 1;
        }
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    // a component that was not updated is not copied back: the caller's array keeps its bits
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (hq / hf have been read: they take the results)
    if (flags & SNPM_ADMIX_UPDATE_Q) HIPCHK(ctx, hipMemcpyAsync(hq.data(), d_q[at_q], q_doubles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (flags & SNPM_ADMIX_UPDATE_F) HIPCHK(ctx, hipMemcpyAsync(hf.data(), d_f[at_f], f_doubles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(loglik, d_out, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx are read until here)
    if (flags & SNPM_ADMIX_UPDATE_Q)
        for (int64_t i = 0; i < ncols; ++i) memcpy(Q + i * K, &hq[(size_t)i * kt], (size_t)K * sizeof(double));
    if (flags & SNPM_ADMIX_UPDATE_F)
        for (int64_t s = 0; s < n_rows; ++s) memcpy(F + s * K, &hf[(size_t)s * kt], (size_t)K * sizeof(double));
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
