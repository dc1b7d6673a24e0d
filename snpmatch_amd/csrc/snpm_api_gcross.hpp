// snpm_api_gcross.hpp -- C ABI: genotype_cross -- parental calls of every (genome window, F2 sample) in one device call (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- genotype_cross
// Everything is validated on the host BEFORE the context is looked at or the device touched (a NULL context then reports what is
// wrong with the arguments through snpm_last_error(NULL), and only a call with sound arguments asks for a context): the kernel
// indexes with win_off and p1 / p2 as they come.
int snpm_cross_calls(snpm_ctx *ctx, const uint8_t *gt_codes, int64_t n, int n_samples, int64_t ld, const int8_t *p1, const int8_t *p2,
                     const int64_t *win_off, int n_win, double lr_thres, int n_marker_thres, int8_t *geno, int32_t *counts)
{
    CHECK_ARG(ctx, n >= 0 && n_samples >= 0 && n_win >= 0 && ld >= 0, "negative size");
    CHECK_ARG(ctx, ld >= n_samples, "ld smaller than n_samples");
    CHECK_ARG(ctx, (int64_t)n_samples <= (int64_t)65535 * GC_TILE, "too many samples for one call");
    CHECK_ARG(ctx, lr_thres == lr_thres, "lr_thres is NaN");
    if (n_win > 0)
        if (int bad = check_offsets(ctx, "win_off", win_off, n_win, n, INT32_MAX, "a window holds more than 2^31 - 1 markers")) return bad;
    if (n > 0) {
        CHECK_ARG(ctx, p1 != nullptr && p2 != nullptr, "p1 / p2 is NULL");
        for (int64_t r = 0; r < n; ++r) {
            CHECK_ARG(ctx, p1[r] >= 0 && p1[r] <= 2 && p2[r] >= 0 && p2[r] <= 2, "parental calls must be 0, 1 or 2");
            CHECK_ARG(ctx, p1[r] != p2[r], "the parents must differ at every marker");
        }
        if (n_samples > 0) {
            CHECK_ARG(ctx, gt_codes != nullptr, "gt_codes is NULL");
            for (int64_t r = 0; r < n; ++r) {
                const uint8_t *row = gt_codes + r * ld;
                bool ok = true;
                for (int s = 0; s < n_samples; ++s) ok &= gt_code_defined(row[s]);
                CHECK_ARG(ctx, ok, "a genotype code outside the defined ones (0xFF: a genotype without a separator)");
            }
        }
    }
    if (n_win == 0 || n_samples == 0) return SNPM_OK;                // nothing to write, nothing launched
    CHECK_ARG(ctx, geno != nullptr, "geno is NULL");
    const size_t cells = (size_t)n_win * (size_t)n_samples;
    if (n == 0) {                                                    // every window is empty: 'NA' everywhere, nothing launched
        memset(geno, 0xFF, cells);
        if (counts) memset(counts, 0, cells * 3 * sizeof(int32_t));
        return SNPM_OK;
    }
    if (!ctx) return set_err(nullptr, SNPM_ERR_BADARG, "ctx is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t pitch = ((int64_t)n_samples + 255) / 256 * 256;    // the kernel loads 4 bytes per lane: rows aligned and padded in the library's own buffer
    int rc;
    if ((rc = ensure(ctx, ctx->ws_gc_codes, (size_t)n * (size_t)pitch))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gc_par, 2 * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gc_off, ((size_t)n_win + 1) * sizeof(int64_t)))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gc_geno, cells))) return rc;
    if (counts && (rc = ensure(ctx, ctx->ws_gc_counts, cells * 3 * sizeof(int32_t)))) return rc;
    int8_t *d_p1 = (int8_t *)ctx->ws_gc_par.p, *d_p2 = d_p1 + n;
    // only the n_samples columns of a row travel: the caller's padding columns never reach the device
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->ws_gc_codes.p, (size_t)pitch, gt_codes, (size_t)ld, (size_t)n_samples, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_p1, p1, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_p2, p2, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ws_gc_off.p, win_off, ((size_t)n_win + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, PK_GCROSS);
        const dim3 grid((unsigned)n_win, (unsigned)((n_samples + GC_TILE - 1) / GC_TILE));
        hipLaunchKernelGGL(k_gcross, grid, dim3(GC_THREADS), 0, ctx->stream, (const uint8_t *)ctx->ws_gc_codes.p, pitch, n_samples,
                           (const int8_t *)d_p1, (const int8_t *)d_p2, (const int64_t *)ctx->ws_gc_off.p, lr_thres, n_marker_thres,
                           (int8_t *)ctx->ws_gc_geno.p, counts ? (int32_t *)ctx->ws_gc_counts.p : nullptr);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(geno, ctx->ws_gc_geno.p, cells, hipMemcpyDeviceToHost, ctx->stream));
    if (counts) HIPCHK(ctx, hipMemcpyAsync(counts, ctx->ws_gc_counts.p, cells * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SNPM_OK;
}
