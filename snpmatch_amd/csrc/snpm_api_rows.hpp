// snpm_api_rows.hpp -- what the table calls (pairsnp, genotype_cross, its HMM) and the panel scans (kinship, site statistics, LD) share on the host: the check of an offset table, of a row's genotype codes, of a row selection, the scratch of a scan and the walk over row slabs (inside the anonymous namespace of snpm_api.hip).
// Part of the one translation unit of libsnpmatch_hip.so: included by snpm_api.hip at this place, not on its own.
// Every check only reads host memory and reports through set_err: a caller runs it before the device is touched.

// A table of k + 1 offsets (`name` in the messages): not NULL, starts at 0, never decreases, ends at n (n < 0: any end).  The
// faults of an entry are reported in table order, so an entry wider than `span_max` is refused -- with `span_msg` -- before a
// later entry that decreases.
int check_offsets(snpm_ctx *ctx, const char *name, const int64_t *off, int64_t k, int64_t n, int64_t span_max = INT64_MAX, const char *span_msg = "")
{
    if (!off) return set_err(ctx, SNPM_ERR_BADARG, "%s is NULL", name);
    if (off[0] != 0) return set_err(ctx, SNPM_ERR_BADARG, "%s must start at 0", name);
    for (int64_t i = 0; i < k; ++i) {
        if (off[i + 1] < off[i]) return set_err(ctx, SNPM_ERR_BADARG, "%s must not decrease", name);
        if (off[i + 1] - off[i] > span_max) return set_err(ctx, SNPM_ERR_BADARG, "%s", span_msg);
    }
    if (n >= 0 && off[k] != n) return set_err(ctx, SNPM_ERR_BADARG, "%s must end at n", name);
    return SNPM_OK;
}

// a genotype code of genotype_cross and its HMM: allele fields 0..4, no bit above them (0xFF: a genotype without a separator)
inline bool gt_code_defined(uint8_t code) { return (code & 7u) <= 4u && (code & 0xF0u) == 0; }

// the row selection of a panel scan: a list of n_rows panel rows (any order, repeats allowed), or the range [row0, row0 + n_rows)
int check_rows(snpm_ctx *ctx, const snpm_panel *p, const int64_t *row_idx, int64_t row0, int64_t n_rows)
{
    if (row_idx) {
        for (int64_t r = 0; r < n_rows; ++r) CHECK_ARG(ctx, row_idx[r] >= 0 && row_idx[r] < p->n_snp, "row index outside the panel");
    } else {
        CHECK_ARG(ctx, row0 >= 0 && row0 <= p->n_snp && n_rows <= p->n_snp - row0, "row range outside the panel");
    }
    return SNPM_OK;
}

// The device scratch of one panel scan (snpm_scratch.hpp): all parts of `s` in ctx->ws_scan, which grows to the largest call.
int scratch_commit(snpm_ctx *ctx, Scratch &s)
{
    if (!s.ok()) return set_err(ctx, SNPM_ERR_OOM, "the device scratch of this call does not fit the address space");
    if (int rc = ensure(ctx, ctx->ws_scan, s.total())) return rc;
    s.assign(ctx->ws_scan.p);
    return SNPM_OK;
}

// The selected rows, `slab_rows` at a time: body(d_rows, first, s0, n_valid) queues the work of slab rows [s0, s0 + n_valid), whose
// row k is panel row d_rows[first + k], or first + k for a range (d_rows null).  A row list travels slab by slab into `d_rows`, the
// caller's scratch part of min(slab_rows + halo, n_rows) entries, null without a list (stream order: the previous slab's kernel
// has read its part before this copy lands).  The caller's row_idx is read until the stream is synchronised.
// halo: rows BEHIND a slab that its work reads as well (the band of snpm_panel_ld_band): the list of a slab then holds up to
// n_valid + halo rows, as far as the selection goes.
template <class Body>
int for_each_row_slab(snpm_ctx *ctx, const int64_t *row_idx, int64_t *d_rows, int64_t row0, int64_t n_rows, int64_t slab_rows, Body body, int64_t halo = 0)
{
    for (int64_t s0 = 0; s0 < n_rows; s0 += slab_rows) {
        const int64_t n_valid = std::min(slab_rows, n_rows - s0);
        if (row_idx) HIPCHK(ctx, hipMemcpyAsync(d_rows, row_idx + s0, (size_t)std::min(n_valid + halo, n_rows - s0) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
        if (int rc = body(row_idx ? d_rows : nullptr, row_idx ? (int64_t)0 : row0 + s0, s0, n_valid)) return rc;
    }
    return SNPM_OK;
}
