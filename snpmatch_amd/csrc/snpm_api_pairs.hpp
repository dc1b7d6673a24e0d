// snpm_api_pairs.hpp -- C ABI: pairsnp -- common / matching record counts of every pair of samples, per segment, in one device call (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- pairsnp
// As snpm_cross_calls: everything is validated on the host BEFORE the context is looked at or the device touched.  The kernels
// rely on ids <= 127 (a larger byte would carry into its neighbour in the byte-parallel tests) and on the chunk table built here.
int snpm_pair_counts(snpm_ctx *ctx, const uint8_t *ids, int64_t n, int n_samples, int64_t ld, const int64_t *seg_off, int n_seg,
                     int32_t *common, int32_t *match)
{
    CHECK_ARG(ctx, n >= 0 && n_samples >= 0 && n_seg >= 0 && ld >= 0, "negative size");
    CHECK_ARG(ctx, ld >= n_samples, "ld smaller than n_samples");
    CHECK_ARG(ctx, n_samples <= SNPM_PAIR_MAX_SAMPLES, "too many samples for one call (SNPM_PAIR_MAX_SAMPLES)");
    CHECK_ARG(ctx, (int64_t)n_seg * n_samples * n_samples <= SNPM_PAIR_MAX_CELLS, "n_seg * n_samples^2 above SNPM_PAIR_MAX_CELLS: split the segments over several calls");
    if (n_seg > 0) {
        if (int bad = check_offsets(ctx, "seg_off", seg_off, n_seg, n, INT32_MAX, "a segment holds 2^31 records or more: its counts would not fit int32")) return bad;
    } else {
        CHECK_ARG(ctx, n == 0, "seg_off must end at n");
    }
    if (n > 0 && n_samples > 0) {
        CHECK_ARG(ctx, ids != nullptr, "ids is NULL");
        for (int64_t r = 0; r < n; ++r) {
            const uint8_t *row = ids + r * ld;
            unsigned high = 0;
            for (int s = 0; s < n_samples; ++s) high |= row[s];
            CHECK_ARG(ctx, (high & 0x80u) == 0, "an id above 127");
        }
    }
    if (n_seg == 0 || n_samples == 0) return SNPM_OK;                // nothing to write, nothing launched
    CHECK_ARG(ctx, common != nullptr && match != nullptr, "common / match is NULL");
    const size_t cells = (size_t)n_seg * (size_t)n_samples * (size_t)n_samples;
    if (n == 0) {                                                    // every segment is empty: zero counts, nothing launched
        memset(common, 0, cells * sizeof(int32_t));
        memset(match, 0, cells * sizeof(int32_t));
        return SNPM_OK;
    }
    if (!ctx) return set_err(nullptr, SNPM_ERR_BADARG, "ctx is NULL");
    try {
        // the padded record axis: every segment starts a chunk and ends with one; an empty segment has none
        std::vector<int64_t> chunk_src;
        std::vector<int32_t> chunk_cnt, chunk_seg;
        for (int s = 0; s < n_seg; ++s)
            for (int64_t r = seg_off[s]; r < seg_off[s + 1]; r += PR_CHUNK) {
                chunk_src.push_back(r);
                chunk_cnt.push_back((int32_t)std::min<int64_t>(PR_CHUNK, seg_off[s + 1] - r));
                chunk_seg.push_back(s);
            }
        const size_t n_chunks = chunk_src.size();
        CHECK_ARG(ctx, n_chunks * (PR_CHUNK / PR_TR_RECORDS) <= (size_t)INT32_MAX, "too many records for one call");
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const int64_t rows = ((int64_t)n_samples + PR_TR_SAMPLES - 1) / PR_TR_SAMPLES * PR_TR_SAMPLES;     // sample rows of the planes (whole transpose tiles)
        const int64_t n_pad = (int64_t)n_chunks * PR_CHUNK;
        const int n_tiles = (n_samples + PR_TILE - 1) / PR_TILE;
        int rc;
        if ((rc = ensure(ctx, ctx->ws_pr_ids, (size_t)n * (size_t)n_samples))) return rc;
        if ((rc = ensure(ctx, ctx->ws_pr_planes, (size_t)rows * (size_t)n_pad))) return rc;
        if ((rc = ensure(ctx, ctx->ws_pr_chunks, n_chunks * 16))) return rc;
        if ((rc = ensure(ctx, ctx->ws_pr_out, 2 * cells * sizeof(int32_t)))) return rc;
        int64_t *d_src = (int64_t *)ctx->ws_pr_chunks.p;
        int32_t *d_cnt = (int32_t *)(d_src + n_chunks), *d_seg = d_cnt + n_chunks;
        int32_t *d_common = (int32_t *)ctx->ws_pr_out.p, *d_match = d_common + cells;
        // only the n_samples columns of a row travel, packed: the caller's padding columns never reach the device
        if (ld == n_samples)
            HIPCHK(ctx, hipMemcpyAsync(ctx->ws_pr_ids.p, ids, (size_t)n * (size_t)n_samples, hipMemcpyHostToDevice, ctx->stream));
        else
            HIPCHK(ctx, hipMemcpy2DAsync(ctx->ws_pr_ids.p, (size_t)n_samples, ids, (size_t)ld, (size_t)n_samples, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_src, chunk_src.data(), n_chunks * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_cnt, chunk_cnt.data(), n_chunks * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_seg, chunk_seg.data(), n_chunks * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_common, 0, 2 * cells * sizeof(int32_t), ctx->stream));
        {
            ProfScope ps(ctx, PK_PAIRS_T);
            const dim3 grid((unsigned)(n_chunks * (PR_CHUNK / PR_TR_RECORDS)), (unsigned)(rows / PR_TR_SAMPLES));
            hipLaunchKernelGGL(k_pair_transpose, grid, dim3(PR_THREADS), 0, ctx->stream, (const uint8_t *)ctx->ws_pr_ids.p, (int64_t)n_samples, n_samples,
                               (const int64_t *)d_src, (const int32_t *)d_cnt, (uint8_t *)ctx->ws_pr_planes.p, n_pad);
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_PAIRS_C);
            const dim3 grid((unsigned)n_chunks, (unsigned)(n_tiles * (n_tiles + 1) / 2));
            hipLaunchKernelGGL(k_pair_count, grid, dim3(PR_THREADS), 0, ctx->stream, (const uint8_t *)ctx->ws_pr_planes.p, n_pad, n_samples,
                               n_tiles, (const int32_t *)d_seg, d_common, d_match);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipMemcpyAsync(common, d_common, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(match, d_match, cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));             // (the chunk table above lives until here)
        return SNPM_OK;
    }
    SNPM_GUARD(ctx)
}
