// snpm_api_ld.hpp -- C ABI: panel LD -- the nine pair counts and r2 of every selected panel row with each of the `band` rows after it, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- LD band
// As snpm_panel_site_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernels rely on every row
// index lying inside the panel and on membership bits at or beyond n_acc being zero.
//
// Slabs: the row axis is cut so that the planes and the outputs of a slab fit the workspace budget (SNPM_LD_WS_MB): ld_slab_rows of
// snpm_k_ld.hpp.  A slab of rows [s0, s0 + n_valid) pairs its rows with rows up to s0 + n_valid + band: for_each_row_slab carries
// that halo, so a row list travels slab by slab with the halo rows behind it.  Two launches per slab; its cells are copied to the
// caller's arrays (whole rows: contiguous) before the next slab's launches overwrite the workspaces (stream order).
int snpm_panel_ld_band(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                       int64_t band, int32_t v_alt, int32_t v_het, int32_t min_n, int32_t *counts, double *r2)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, band >= 1 && band <= SNPM_LD_MAX_BAND, "band must be 1 .. SNPM_LD_MAX_BAND");
    CHECK_ARG(ctx, v_alt >= 0 && v_alt <= 3 && v_het >= 0 && v_het <= 3, "v_alt and v_het must be 0 .. 3");
    CHECK_ARG(ctx, min_n >= 1, "min_n must be at least 1");
    if (n_rows > 0) CHECK_ARG(ctx, counts != nullptr || r2 != nullptr, "counts and r2 are both NULL");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    const int64_t words = (p->n_acc + 31) / 32;
    std::vector<uint32_t> member((size_t)words, 0u), ordered((size_t)words, 0u);
    if (cols) {
        for (int64_t i = 0; i < ncols; ++i) {
            const int64_t c = cols[i];
            CHECK_ARG(ctx, c >= 0 && c < p->n_acc, "accession index outside the panel");
            uint32_t &w = member[(size_t)(c >> 5)];
            CHECK_ARG(ctx, !((w >> (c & 31)) & 1u), "an accession is listed twice");
            w |= 1u << (c & 31);
        }
    } else {
        for (int64_t c = 0; c < p->n_acc; ++c) member[(size_t)(c >> 5)] |= 1u << (c & 31);
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    CHECK_ARG(ctx, p->n_acc <= LD_MAX_ACCESSIONS, "the panel is wider than 16384 accessions");
    if (n_rows == 0) return SNPM_OK;                                // nothing to write, nothing launched
    for (int64_t w = 0; w < words; ++w) ordered[(size_t)w] = site_member_word(member.data(), words, p->packed != 0, 0, (int)w, 0);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t slab_rows = ld_slab_rows(ctx->ld_ws_bytes, words, band, n_rows), plane_rows = std::min(slab_rows + band, n_rows);
    Scratch sc;                                                      // membership words; planes [slab rows + band][3][words]; counts and r2 of a slab; row list with its halo
    uint32_t *d_member, *d_planes;
    int32_t *d_counts = nullptr;
    double *d_r2 = nullptr;
    int64_t *d_rowlist = nullptr;
    sc.want(d_member, (size_t)words);
    sc.want(d_planes, (size_t)plane_rows * 3 * (size_t)words);
    if (counts) sc.want(d_counts, (size_t)slab_rows * (size_t)band * 9);
    if (r2) sc.want(d_r2, (size_t)slab_rows * (size_t)band);
    if (row_idx) sc.want(d_rowlist, (size_t)plane_rows);
    if ((rc = scratch_commit(ctx, sc))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_member, ordered.data(), (size_t)words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const bool wide = site_wide_rows(p->d, p->kpitch, p->desc);      // every panel the library makes, except split rows with a tail below 16 bytes
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, slab_rows, [&](const int64_t *d_rows, int64_t first, int64_t s0, int64_t n_valid) {
        const int64_t n_plane = std::min(n_valid + band, n_rows - s0);      // the slab's rows and its halo, as far as the selection goes
        {
            ProfScope ps(ctx, PK_LD_P);
            const int64_t blocks = (n_plane * words + LD_PLANE_THREADS - 1) / LD_PLANE_THREADS;
            const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)ctx->n_cu * 16)));
#define SNPM_LD_LAUNCH(PK, WD)                                                                                                    \
    hipLaunchKernelGGL((k_ld_planes<PK, WD>), grid, dim3(LD_PLANE_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, p->n_acc, \
                       d_rows, first, n_plane, (const uint32_t *)d_member, (int)words, d_planes)
            if (p->packed) { if (wide) SNPM_LD_LAUNCH(true, true); else SNPM_LD_LAUNCH(true, false); }
            else { if (wide) SNPM_LD_LAUNCH(false, true); else SNPM_LD_LAUNCH(false, false); }
#undef SNPM_LD_LAUNCH
            HIPCHK(ctx, hipGetLastError());
        }
        {
            ProfScope ps(ctx, PK_LD_B);
            const dim3 grid((unsigned)((n_valid + LD_T - 1) / LD_T), (unsigned)((band + LD_D - 1) / LD_D));
            hipLaunchKernelGGL(k_ld_band, grid, dim3(LD_THREADS), 0, ctx->stream, (const uint32_t *)d_planes, (int)words, n_plane, n_valid, band,
                               (int)v_alt, (int)v_het, (int)min_n, d_counts, d_r2);
            HIPCHK(ctx, hipGetLastError());
        }
        if (counts) HIPCHK(ctx, hipMemcpyAsync(counts + s0 * band * 9, d_counts, (size_t)(n_valid * band) * 9 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (r2) HIPCHK(ctx, hipMemcpyAsync(r2 + s0 * band, d_r2, (size_t)(n_valid * band) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        return (int)SNPM_OK;
    }, band);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's row_idx and `ordered` are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
