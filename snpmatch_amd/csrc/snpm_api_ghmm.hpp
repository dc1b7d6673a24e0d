// snpm_api_ghmm.hpp -- C ABI: genotype_cross_hmm -- the Viterbi path of every (chain, F2 sample) in one device call (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- genotype_cross_hmm
// As snpm_cross_calls: everything is validated on the host BEFORE the context is looked at or the device touched -- the kernel
// indexes the tables with pair, depth_rank and the codes as they come, and walks the rows chain_off names.
int snpm_cross_hmm(snpm_ctx *ctx, const uint8_t *gt_codes, const uint16_t *depth_rank, int64_t n, int n_samples, int64_t ld,
                   const uint8_t *pair, const int64_t *chain_off, int n_chain, const double *logT, const double *logI,
                   const double *logE, int n_depth, int8_t *state, double *omega)
{
    CHECK_ARG(ctx, n >= 0 && n_samples >= 0 && n_chain >= 0 && ld >= 0 && n_depth >= 0, "negative size");
    CHECK_ARG(ctx, ld >= n_samples, "ld smaller than n_samples");
    CHECK_ARG(ctx, (int64_t)n_samples <= (int64_t)65535 * WAVE, "too many samples for one call");
    CHECK_ARG(ctx, n_depth <= 65536, "n_depth above 65536: a depth rank is 16 bits wide");
    if (n_chain > 0) {
        if (int bad = check_offsets(ctx, "chain_off", chain_off, n_chain, n)) return bad;
        CHECK_ARG(ctx, logT != nullptr, "logT is NULL");
        for (int64_t k = 0; k < (int64_t)n_chain * 9; ++k) CHECK_ARG(ctx, logT[k] == logT[k] && logT[k] != __builtin_inf(), "NaN or +inf in logT");
    } else {
        CHECK_ARG(ctx, n == 0, "chain_off must end at n");
    }
    if (n > 0) {
        CHECK_ARG(ctx, n_depth >= 1, "n_depth must be at least 1 when there are markers");
        CHECK_ARG(ctx, pair != nullptr, "pair is NULL");
        for (int64_t r = 0; r < n; ++r) CHECK_ARG(ctx, pair[r] < 6, "pair must be below 6 (the ordered pairs of distinct calls 0 / 1 / 2)");
        CHECK_ARG(ctx, logI != nullptr && logE != nullptr, "logI / logE is NULL");
        const int64_t cells = (int64_t)6 * n_depth * 12;
        for (int64_t k = 0; k < cells; ++k) {
            CHECK_ARG(ctx, logI[k] == logI[k] && logI[k] != __builtin_inf(), "NaN or +inf in logI");
            CHECK_ARG(ctx, logE[k] == logE[k] && logE[k] != __builtin_inf(), "NaN or +inf in logE");
        }
        if (n_samples > 0) {
            CHECK_ARG(ctx, gt_codes != nullptr && depth_rank != nullptr, "gt_codes / depth_rank is NULL");
            for (int64_t r = 0; r < n; ++r) {
                const uint8_t *row = gt_codes + r * ld;
                const uint16_t *drow = depth_rank + r * ld;
                bool ok = true, dok = true;
                for (int s = 0; s < n_samples; ++s) {
                    ok &= gt_code_defined(row[s]);
                    dok &= (int)drow[s] < n_depth;
                }
                CHECK_ARG(ctx, ok, "a genotype code outside the defined ones (0xFF: a genotype without a separator)");
                CHECK_ARG(ctx, dok, "a depth_rank at or above n_depth");
            }
        }
    }
    if (n == 0 || n_chain == 0 || n_samples == 0) return SNPM_OK;    // nothing to write, nothing launched
    CHECK_ARG(ctx, state != nullptr, "state is NULL");
    if (!ctx) return set_err(nullptr, SNPM_ERR_BADARG, "ctx is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // rows of the library's own buffers: whole tiles of 64 samples, so every active lane's element lies inside its row
    const int64_t pitch = ((int64_t)n_samples + 63) / 64 * 64;
    const size_t cells = (size_t)n * (size_t)pitch;
    const size_t table = (size_t)6 * (size_t)n_depth * 12 * sizeof(double);
    const size_t om_bytes = (size_t)n * (size_t)n_samples * 3 * sizeof(double);
    int rc;
    if ((rc = ensure(ctx, ctx->ws_gh_codes, cells))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gh_depth, cells * sizeof(uint16_t)))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gh_bp, cells))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gh_state, cells))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gh_pair, (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gh_off, ((size_t)n_chain + 1) * sizeof(int64_t)))) return rc;
    if ((rc = ensure(ctx, ctx->ws_gh_tab, (size_t)n_chain * 9 * sizeof(double) + 2 * table))) return rc;
    if (omega && (rc = ensure(ctx, ctx->ws_gh_omega, om_bytes))) return rc;
    double *d_T = (double *)ctx->ws_gh_tab.p, *d_I = d_T + (size_t)n_chain * 9, *d_E = d_I + (size_t)6 * (size_t)n_depth * 12;
    // only the n_samples columns of a row travel: the caller's padding columns never reach the device
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->ws_gh_codes.p, (size_t)pitch, gt_codes, (size_t)ld, (size_t)n_samples, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->ws_gh_depth.p, (size_t)pitch * sizeof(uint16_t), depth_rank, (size_t)ld * sizeof(uint16_t),
                                 (size_t)n_samples * sizeof(uint16_t), (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ws_gh_pair.p, pair, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ws_gh_off.p, chain_off, ((size_t)n_chain + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_T, logT, (size_t)n_chain * 9 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_I, logI, table, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_E, logE, table, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, PK_GHMM);
        const dim3 grid((unsigned)n_chain, (unsigned)(pitch / WAVE));
        hipLaunchKernelGGL(k_ghmm, grid, dim3(WAVE), 0, ctx->stream, (const uint8_t *)ctx->ws_gh_codes.p, (const uint16_t *)ctx->ws_gh_depth.p,
                           pitch, n_samples, (const uint8_t *)ctx->ws_gh_pair.p, (const int64_t *)ctx->ws_gh_off.p, (const double *)d_T,
                           (const double *)d_I, (const double *)d_E, n_depth, (uint8_t *)ctx->ws_gh_bp.p, (int8_t *)ctx->ws_gh_state.p,
                           omega ? (double *)ctx->ws_gh_omega.p : nullptr);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpy2DAsync(state, (size_t)n_samples, ctx->ws_gh_state.p, (size_t)pitch, (size_t)n_samples, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (omega) HIPCHK(ctx, hipMemcpyAsync(omega, ctx->ws_gh_omega.p, om_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SNPM_OK;
}
