// snpm_api_site.hpp -- C ABI: site statistics -- c0 / c1 / c2 / ninfo of every selected panel row per group of accession columns, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- site counts
// As snpm_panel_kinship_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.  The kernel relies on every row
// index lying inside the panel and on membership bits at or beyond n_acc being zero.
//
// Slabs: the row axis is cut so that the counts of a slab, 16 bytes per (group, row), fit the workspace budget (SNPM_SITE_WS_MB):
// site_slab_rows of snpm_k_site.hpp.  One launch per slab (for_each_row_slab); its counts are copied to the caller's array before
// the next slab's launch overwrites the workspace (stream order); a row list travels slab by slab.
int snpm_panel_site_counts(snpm_panel *panel, const int32_t *cols, const int64_t *grp_off, int64_t n_groups, const int64_t *row_idx,
                           int64_t row0, int64_t n_rows, int32_t *counts)
try {
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, n_groups >= 0 && n_rows >= 0, "negative size");
    CHECK_ARG(ctx, n_groups <= SNPM_SITE_MAX_GROUPS, "too many groups for one call (SNPM_SITE_MAX_GROUPS)");
    if (cols || grp_off) {
        CHECK_ARG(ctx, grp_off != nullptr, "grp_off is NULL with a column list");
        if (int bad = check_offsets(ctx, "grp_off", grp_off, n_groups, -1)) return bad;      // (any end: the columns listed)
        CHECK_ARG(ctx, cols != nullptr || grp_off[n_groups] == 0, "cols is NULL but grp_off lists columns");
    } else {
        CHECK_ARG(ctx, n_groups <= 1, "cols is NULL (all accessions): n_groups must be 1");
    }
    if (n_groups > 0 && n_rows > 0) CHECK_ARG(ctx, counts != nullptr, "counts is NULL");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    const int64_t nwords = (p->n_acc + 31) / 32;
    std::vector<uint32_t> member((size_t)(n_groups * nwords), 0u);
    bool any_member = false;
    if (grp_off) {
        for (int64_t g = 0; g < n_groups; ++g)
            for (int64_t i = grp_off[g]; i < grp_off[g + 1]; ++i) {
                const int64_t c = cols[i];
                CHECK_ARG(ctx, c >= 0 && c < p->n_acc, "accession index outside the panel");
                uint32_t &w = member[(size_t)(g * nwords + (c >> 5))];
                CHECK_ARG(ctx, !((w >> (c & 31)) & 1u), "an accession is listed twice in one group");
                w |= 1u << (c & 31);
                any_member = true;
            }
    } else if (n_groups == 1) {
        for (int64_t c = 0; c < p->n_acc; ++c) member[(size_t)(c >> 5)] |= 1u << (c & 31);
        any_member = true;
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    int lg_s = 0, cpl = 0;
    CHECK_ARG(ctx, site_geometry(p->n_acc, p->packed != 0, &lg_s, &cpl), "the panel is wider than one wave's words (16384 accessions)");
    if (n_groups == 0 || n_rows == 0) return SNPM_OK;               // nothing to write, nothing launched
    if (!any_member) {                                              // empty groups only: zero counts, nothing launched
        memset(counts, 0, (size_t)n_groups * (size_t)n_rows * 4 * sizeof(int32_t));
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t slab_rows = site_slab_rows(ctx->site_ws_bytes, n_groups, n_rows);
    Scratch sc;                                                       // counts [groups][slab rows][4]; membership bitmasks [groups][words]; row list
    int32_t *d_out;
    uint32_t *d_member;
    int64_t *d_rowlist = nullptr;
    sc.want(d_out, (size_t)n_groups * (size_t)slab_rows * 4);
    sc.want(d_member, member.size());
    if (row_idx) sc.want(d_rowlist, (size_t)std::min(slab_rows, n_rows));
    if ((rc = scratch_commit(ctx, sc))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_member, member.data(), member.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const int rpw = WAVE >> lg_s, waves = SITE_THREADS / WAVE;
    const bool wide = site_wide_rows(p->d, p->kpitch, p->desc);      // every panel the library makes, except split rows with a tail below 16 bytes
    rc = for_each_row_slab(ctx, row_idx, d_rowlist, row0, n_rows, slab_rows, [&](const int64_t *d_rows, int64_t first, int64_t s0, int64_t n_valid) {
        {
            ProfScope ps(ctx, PK_SITE);
            const int64_t batches = (n_valid + rpw - 1) / rpw;
            const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((batches + waves - 1) / waves, (int64_t)ctx->n_cu * 2)));
#define SNPM_SITE_LAUNCH(PK, WD)                                                                                                  \
    hipLaunchKernelGGL((k_site_counts<PK, WD>), grid, dim3(SITE_THREADS), 0, ctx->stream, (const int8_t *)p->d, p->kpitch, p->desc, p->n_acc, \
                       d_rows, first, n_valid, (const uint32_t *)d_member, (int)n_groups, lg_s, cpl, d_out)
            if (p->packed) { if (wide) SNPM_SITE_LAUNCH(true, true); else SNPM_SITE_LAUNCH(true, false); }
            else { if (wide) SNPM_SITE_LAUNCH(false, true); else SNPM_SITE_LAUNCH(false, false); }
#undef SNPM_SITE_LAUNCH
            HIPCHK(ctx, hipGetLastError());
        }
        for (int64_t g = 0; g < n_groups; ++g)                       // the slab's [g][n_valid][4] into the caller's [g][n_rows][4]
            HIPCHK(ctx, hipMemcpyAsync(counts + (g * n_rows + s0) * 4, d_out + g * n_valid * 4, (size_t)n_valid * 16, hipMemcpyDeviceToHost, ctx->stream));
        return (int)SNPM_OK;
    });
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's row_idx and `member` are read until here)
    return SNPM_OK;
} SNPM_GUARD((panel ? panel->ctx : nullptr))
