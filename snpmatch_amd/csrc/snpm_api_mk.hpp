// snpm_api_mk.hpp -- C ABI: markers -- a greedy minimal set of panel rows (SNPs) that separates every pair of accession columns `depth` times, on the resident panel (inside the extern "C" block of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// ---------------------------------------------------------------------------------------------- markers
// As snpm_panel_kinship_counts: everything is validated on the host BEFORE the device is touched; what does not need the panel is
// checked before the panel handle is looked at, so those refusals are reachable without a device.
//
// No slabs: the row planes of ALL selected rows (k_mk_rowplanes, 2 bits per call) stay on the device for the whole loop -- a slab
// walk per round would read the panel again every round -- and must fit SNPM_MK_WS_MB.  All rounds run inside this one call as plain
// launches on the context's stream: per round k_mk_gain, k_mk_pick, k_mk_update, enqueued MK_ROUND_BATCH rounds at a time; between
// two batches the host reads the 32-byte MkState and stops when the device has.  The rounds of a batch behind the end of the loop
// return at their first instruction.  No gain vector travels to the host per round (the gains of round 0 once, when the caller
// asks for first_gain).  The loop is bounded by min(max_markers, n_rows) rounds: every round that does not end the loop picks a row,
// and a row is picked once.
int snpm_panel_marker_select(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                             const int64_t *coord, int64_t min_dist, const uint8_t *eligible, int32_t depth, int64_t max_markers,
                             int64_t *chosen, int32_t *gain_at, int64_t *n_chosen, int64_t *remaining, int32_t *stop_reason, uint8_t *need,
                             int32_t *first_gain)
{
    snpm_ctx *ctx = panel ? panel->ctx : nullptr;
    CHECK_ARG(ctx, ncols >= 0 && n_rows >= 0 && max_markers >= 0, "negative size");
    CHECK_ARG(ctx, depth >= 1 && depth <= 255, "depth must lie in 1 .. 255");
    CHECK_ARG(ctx, min_dist >= 0, "min_dist must not be negative");
    CHECK_ARG(ctx, coord != nullptr || min_dist == 0, "min_dist needs coord: without coordinates it must be 0");
    CHECK_ARG(ctx, ncols <= SNPM_MK_MAX_ACCESSIONS, "too many accessions for one call (SNPM_MK_MAX_ACCESSIONS)");
    CHECK_ARG(ctx, n_rows <= INT32_MAX, "2^31 rows or more: a position would not fit the pick key");
    CHECK_ARG(ctx, n_chosen != nullptr && remaining != nullptr && stop_reason != nullptr, "n_chosen / remaining / stop_reason is NULL");
    const int64_t cap = std::min(max_markers, n_rows);               // rounds at most, and entries of chosen / gain_at written at most
    if (ncols > 0) CHECK_ARG(ctx, need != nullptr, "need is NULL");
    if (cap > 0) CHECK_ARG(ctx, chosen != nullptr && gain_at != nullptr, "chosen / gain_at is NULL");
    CHECK_PANEL(panel);
    snpm_panel *p = panel;
    if (cols) {
        for (int64_t a = 0; a < ncols; ++a) CHECK_ARG(ctx, cols[a] >= 0 && cols[a] < p->n_acc, "accession index outside the panel");
    } else {
        CHECK_ARG(ctx, ncols == 0 || ncols == p->n_acc, "cols is NULL (all accessions): ncols must be the panel's accession count");
    }
    if (int bad = check_rows(ctx, p, row_idx, row0, n_rows)) return bad;
    const int64_t cols_pad = (ncols + WAVE - 1) / WAVE * WAVE;
    const int Wc = (int)(cols_pad / WAVE);
    // (fp64: n_rows < 2^31 and cols_pad <= 4096, the product is exact)
    const double planes_need = (double)n_rows * 2.0 * (double)cols_pad / 8.0;
    if (planes_need > (double)ctx->mk_ws_bytes)
        return set_err(ctx, SNPM_ERR_BADARG, "the row planes of %lld candidate rows x %lld accessions need %.0f bytes on the device for the whole loop, more than SNPM_MK_WS_MB allows (%zu bytes): thin the candidates (a site list from sitestats --min_maf / --max_missing or from ld pruning), or a larger SNPM_MK_WS_MB",
                       (long long)n_rows, (long long)ncols, planes_need, ctx->mk_ws_bytes);
    const size_t cells = (size_t)ncols * (size_t)ncols;
    MkState init;
    init.n_chosen = 0;
    init.remaining = (long long)depth * (long long)(ncols * (ncols - 1) / 2);
    init.pick = -1;
    init.done = 0;
    init.reason = 0;
    if (ncols < 2 || n_rows == 0 || max_markers == 0) {              // the initial state, nothing launched
        for (int64_t a = 0; a < ncols; ++a)
            for (int64_t b = 0; b < ncols; ++b) need[a * ncols + b] = a == b ? 0 : (uint8_t)depth;
        if (first_gain && n_rows > 0) memset(first_gain, 0, (size_t)n_rows * sizeof(int32_t));
        *n_chosen = 0;
        *remaining = init.remaining;
        *stop_reason = init.remaining == 0 ? MK_STOP_RESOLVED : max_markers == 0 ? MK_STOP_MAX_MARKERS : MK_STOP_NO_GAIN;
        return SNPM_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    const int64_t n_best = (n_rows + MK_GAIN_ROWS - 1) / MK_GAIN_ROWS;
    Scratch sc;     // row planes [n_rows][2][Wc]; Ut [Wc][cols_pad]; need; gains; block keys; eligibility; chosen | gain_at; MkState; coordinates; column list; row list
    unsigned long long *d_H, *d_Ut, *d_best;
    uint8_t *d_need, *d_elig, *d_picks;
    int32_t *d_gain, *d_cols = nullptr;
    MkState *d_st;
    int64_t *d_coord = nullptr, *d_rows = nullptr;
    sc.want(d_H, (size_t)n_rows * 2 * (size_t)Wc);
    sc.want(d_Ut, (size_t)Wc * (size_t)cols_pad);
    sc.want(d_need, cells);
    sc.want(d_gain, (size_t)n_rows);
    sc.want(d_best, (size_t)n_best);
    sc.want(d_elig, (size_t)n_rows);
    sc.want(d_picks, (size_t)cap * (sizeof(int64_t) + sizeof(int32_t)));
    sc.want(d_st, 1);
    if (coord) sc.want(d_coord, (size_t)n_rows);
    if (cols) sc.want(d_cols, (size_t)ncols);
    if (row_idx) sc.want(d_rows, (size_t)n_rows);
    if ((rc = scratch_commit(ctx, sc))) return rc;
    if ((rc = ensure_pinned(ctx, 2 * sizeof(MkState)))) return rc;
    MkState *h_init = (MkState *)ctx->h_pinned, *h_st = h_init + 1;  // what goes up before the first launch; what comes back between batches
    *h_init = init;
    int64_t *d_chosen = (int64_t *)d_picks;
    int32_t *d_gain_at = (int32_t *)(d_chosen + cap);
    if (cols) HIPCHK(ctx, hipMemcpyAsync(d_cols, cols, (size_t)ncols * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (row_idx) HIPCHK(ctx, hipMemcpyAsync(d_rows, row_idx, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (coord) HIPCHK(ctx, hipMemcpyAsync(d_coord, coord, (size_t)n_rows * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (eligible) HIPCHK(ctx, hipMemcpyAsync(d_elig, eligible, (size_t)n_rows, hipMemcpyHostToDevice, ctx->stream));
    else HIPCHK(ctx, hipMemsetAsync(d_elig, 1, (size_t)n_rows, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_st, h_init, sizeof(MkState), hipMemcpyHostToDevice, ctx->stream));
    const dim3 upd_grid((unsigned)(cols_pad / (MK_THREADS / WAVE)));
    {
        ProfScope ps(ctx, PK_MK_P);
        hipLaunchKernelGGL(k_mk_rowplanes, dim3((unsigned)((n_rows + MK_PL_ROWS - 1) / MK_PL_ROWS)), dim3(MK_THREADS), 0, ctx->stream, (const int8_t *)p->d,
                           p->kpitch, p->desc, d_rows, row_idx ? (int64_t)0 : row0, n_rows, d_cols, (int)ncols, d_H, Wc);
        HIPCHK(ctx, hipGetLastError());
    }
    {
        ProfScope ps(ctx, PK_MK_U);                                  // the initial need and Ut
        hipLaunchKernelGGL(k_mk_update, upd_grid, dim3(MK_THREADS), 0, ctx->stream, (const unsigned long long *)d_H, n_rows, Wc, (int)ncols, cols_pad,
                           (const MkState *)d_st, (int64_t)-1, (int)depth, d_need, d_Ut);
        HIPCHK(ctx, hipGetLastError());
    }
    int64_t round = 0;
    bool done = false;
    while (round < cap && !done) {
        const int64_t upto = std::min(cap, round + MK_ROUND_BATCH);
        for (; round < upto; ++round) {
            {
                ProfScope ps(ctx, PK_MK_G);
                hipLaunchKernelGGL(k_mk_gain, dim3((unsigned)n_best), dim3(MK_THREADS), 0, ctx->stream, (const unsigned long long *)d_H,
                                   (const unsigned long long *)d_Ut, (const uint8_t *)d_elig, (const MkState *)d_st, n_rows, cols_pad, Wc,
                                   (int)(round == 0 && first_gain != nullptr), d_gain, d_best);
                HIPCHK(ctx, hipGetLastError());
            }
            // (stream order: the gains of round 0 leave before round 1 writes its own)
            if (round == 0 && first_gain) HIPCHK(ctx, hipMemcpyAsync(first_gain, d_gain, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            {
                ProfScope ps(ctx, PK_MK_K);
                hipLaunchKernelGGL(k_mk_pick, dim3(1), dim3(MK_PICK_THREADS), 0, ctx->stream, (const unsigned long long *)d_best, n_best, d_elig, d_coord,
                                   min_dist, n_rows, max_markers, cap, d_chosen, d_gain_at, d_st);
                HIPCHK(ctx, hipGetLastError());
            }
            {
                ProfScope ps(ctx, PK_MK_U);
                hipLaunchKernelGGL(k_mk_update, upd_grid, dim3(MK_THREADS), 0, ctx->stream, (const unsigned long long *)d_H, n_rows, Wc, (int)ncols, cols_pad,
                                   (const MkState *)d_st, round, 0, d_need, d_Ut);
                HIPCHK(ctx, hipGetLastError());
            }
        }
        HIPCHK(ctx, hipMemcpyAsync(h_st, d_st, sizeof(MkState), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        done = h_st->done != 0;
    }
    // (the device's own figures are range-checked before they size a copy)
    if (h_st->n_chosen < 0 || h_st->n_chosen > cap) return set_err(ctx, SNPM_ERR_STATE, "internal error: %lld picks in %lld rounds", h_st->n_chosen, (long long)cap);
    const size_t n = (size_t)h_st->n_chosen;
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(chosen, d_chosen, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(gain_at, d_gain_at, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(need, d_need, cells, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                 // (the caller's cols / row_idx / coord / eligible are read until here)
    *n_chosen = h_st->n_chosen;
    *remaining = h_st->remaining;
    // not done after min(max_markers, n_rows) rounds: every row was picked, fewer than max_markers, and pairs are left
    *stop_reason = done ? h_st->reason : MK_STOP_NO_GAIN;
    return SNPM_OK;
}
