// snpm_once.hpp -- ONE sample against a resident panel in ONE call: snpm_genotype_once / snpm_genotype_once_coded
// (Genotyper.genotyper, core/snpmatch.py:207-241, for a single sample).
//
// Every call starts the same way: the host thread pool gathers wei[sample_idx[i]] (or the weight codes) and the row list into
// ONE pinned slab and learns on the way what the kernels are chosen by -- whether every weight is an integer, 0 or 1, finite,
// the sum of max |w| per row, the first bad index (OnceGather).  A bad index, a bad code or a non-finite weight refuses the call
// before a kernel consumes the slab.  Every call ends the same way: 4 n_acc + 2 words {score, ninfo, lik, lrt, flagged count,
// status} lie in the pinned slab and once_read_out hands them to the caller.  In between there are two forms:
//   genotype_once_fused (default)  k_once_prep reads the slab where it lies and prepares everything the scoring needs in one
//      launch; fast pass, reduce + certificate, the sparse tier, k_once_tail (likelihood / nanmin / ratio of the truncated
//      counts, :96, :106-117, + status) written straight into the slab: no copy, one synchronisation.
//   genotype_once_unfused (SNPM_ONCE_FUSED=0, chunk > ONCE_MAX_CHUNK, n == 0)  the slab goes up in pieces behind the fill, then
//      row check / code expansion, the scoring pipeline of snpm_query_run_device, snpm_likelihood_device and k_once_pack as
//      separate launches, one packed copy back.
// Both return the same bits (tests/test_gpu_once.py).  Each form keeps its own rows per fill task: q->wsum is the sum of the
// per-task sums, and the certificate's flag rule reads it.
// Switches: SNPM_ONCE_FUSED=0 (the unfused form for every call), SNPM_ONCE_TAIL=0 (k_scan_few + k_once_finish instead of
// k_once_tail), SNPM_ONCE_TRACE (host-side times of a call on stderr).
// Included by snpm_api.hip inside its extern "C" block.

namespace {          // plain host code, no HIP call: the gather and what it learns

// Properties of one weight.  Bit 0: not an integer, or too large for the integer kernels; bit 1: neither 0 nor 1; bit 2: NaN /
// infinite.  Integer tests on the bit pattern and no branch: the gather of an fp64 sample calls it once per weight.
inline uint32_t once_weight_flags(double v)
{
    uint64_t b;
    memcpy(&b, &v, 8);
    const uint64_t mag = b & 0x7FFFFFFFFFFFFFFFull;
    const double a = fabs(v), small = a < 9.0e15 ? a : 0.0;         // (a select: only a value an int64 holds is converted)
    return (uint32_t)((double)(int64_t)small != small) | (uint32_t)(!(a < 9.0e15)) |
           ((uint32_t)(!((mag == 0) | (b == 0x3FF0000000000000ull))) << 1) | ((uint32_t)(mag >= 0x7FF0000000000000ull) << 2);
}

struct OnceProps {          // per task of the fill
    long double wsum = 0;
    int flags = 0;          // once_weight_flags of every weight, or-ed; bit 3: a weight code past the table
    int64_t bad_row = -1;   // position of a row index outside the panel / a sample index outside the weights
    char pad[64];
};

struct OnceSums {           // ... and over all tasks
    long double tot = 0;
    int flags = 0;
    int64_t bad_at = -1;    // first position with a bad row index, sample index or weight code
};

// The gather of one call.  The slab: [rows int64 | weights fp64 x 3] = 32 B per matched SNP, coded [rows int32 | codes uint16 x 3]
// = 10 B.  Coded samples look their properties up per code (code_flags, code_abs: 65536 entries each, once_set_table).
struct OnceGather {
    const int64_t *row_idx;
    const double *wei;
    const uint16_t *codes;          // not NULL: the coded form
    int64_t table_len;
    const int64_t *sample_idx;
    int64_t n_wei, n, n_snp;
    int64_t piece;                  // rows per fill task
    const uint8_t *code_flags = nullptr;
    const double *code_abs = nullptr;
    char *slab = nullptr;
    size_t row_bytes = 0, wei_bytes = 0;
    std::vector<OnceProps> props;

    bool coded() const { return codes != nullptr; }
    int n_tasks() const { return (int)((n + piece - 1) / piece); }
    int64_t *rows() const { return (int64_t *)slab; }
    int32_t *rows32() const { return (int32_t *)slab; }
    double *weights() const { return (double *)(slab + row_bytes); }
    uint16_t *wcodes() const { return (uint16_t *)(slab + row_bytes); }
    void lay_out()
    {
        row_bytes = ((size_t)n * (coded() ? sizeof(int32_t) : sizeof(int64_t)) + 7) / 8 * 8;
        wei_bytes = (size_t)n * 3 * (coded() ? sizeof(uint16_t) : sizeof(double));
        props.assign((size_t)std::max(n_tasks(), 1), OnceProps());
    }
    void fill(int t)
    {
        const int64_t i0 = (int64_t)t * piece, i1 = std::min<int64_t>(n, i0 + piece);
        int64_t *const h_rows = rows();
        int32_t *const h_rows32 = rows32();
        double *const h_wei = weights();
        uint16_t *const h_codes = wcodes();
        const bool is_coded = coded();
        OnceProps pr;
        double wsum = 0.0;                                         // non-negative terms; the caller rounds the total up
        uint32_t fl = 0;
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t r = row_idx[i];
            if ((uint64_t)r >= (uint64_t)n_snp && pr.bad_row < 0) pr.bad_row = i;
            if (is_coded) h_rows32[i] = (uint64_t)r < (uint64_t)n_snp ? (int32_t)r : -1;
            else h_rows[i] = r;
            int64_t s = sample_idx ? sample_idx[i] : i;
            if ((uint64_t)s >= (uint64_t)n_wei) {                  // a sample index outside the weight array: reported like a bad row
                if (pr.bad_row < 0) pr.bad_row = i;
                s = 0;
            }
            if (is_coded) {
                const uint16_t c0 = codes[3 * s], c1 = codes[3 * s + 1], c2 = codes[3 * s + 2];
                h_codes[3 * i] = c0; h_codes[3 * i + 1] = c1; h_codes[3 * i + 2] = c2;
                fl |= (uint32_t)(code_flags[c0] | code_flags[c1] | code_flags[c2]);
                const double a0 = code_abs[c0], a1 = code_abs[c1], a2 = code_abs[c2];
                const double m01 = a0 > a1 ? a0 : a1;
                wsum += m01 > a2 ? m01 : a2;
            } else {
                double m = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double v = wei[3 * s + c], a = fabs(v);
                    h_wei[3 * i + c] = v;
                    fl |= once_weight_flags(v);
                    m = a > m ? a : m;
                }
                wsum += m;
            }
        }
        pr.wsum = wsum;
        pr.flags = (int)fl;
        props[(size_t)t] = pr;
    }
    OnceSums reduce() const
    {
        OnceSums s;
        for (int t = 0; t < n_tasks(); ++t) {
            if (props[(size_t)t].bad_row >= 0 && s.bad_at < 0) s.bad_at = props[(size_t)t].bad_row;
            s.tot += props[(size_t)t].wsum;
            s.flags |= props[(size_t)t].flags;
        }
        if ((s.flags & 8) && s.bad_at < 0) {                       // a code outside the table: find it for the message
            for (int64_t i = 0; i < n && s.bad_at < 0; ++i) {
                const int64_t k = sample_idx ? sample_idx[i] : i;
                for (int c = 0; c < 3; ++c)
                    if ((int64_t)codes[3 * k + c] >= table_len) s.bad_at = i;
            }
        }
        return s;
    }
};

struct OnceTrace {          // SNPM_ONCE_TRACE: when the fill and the enqueueing of a call were done
    static double now()
    {
        static const bool on = getenv("SNPM_ONCE_TRACE") != nullptr;
        return on ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() : -1.0;
    }
    double t_begin = now(), t_filled = 0, t_enqueued = 0;
    void report(const OnceGather &g, const char *form) const
    {
        if (t_begin >= 0)
            fprintf(stderr, "[snpm once] n %lld: fill %.3f ms (%d tasks), enqueue %.3f ms, wait %.3f ms%s\n", (long long)g.n, t_filled - t_begin,
                    g.n_tasks(), t_enqueued - t_filled, now() - t_enqueued, form);
    }
};

}  // namespace

// The weight table of the coded form on the device (uploaded when it is not the one of the previous call) and, with it, the
// properties of every code: a flag byte and |entry| (65536 of each; codes past the table carry bit 3).  BOTH forms of the call
// go through here: the per-code tables always describe ctx->once_table.
static int once_set_table(snpm_ctx *ctx, const double *table, int64_t table_len)
{
    int rc = ensure(ctx, ctx->ws_once_table, 65536 * sizeof(double));
    if (rc) return rc;
    if (ctx->once_table.size() == (size_t)table_len && ctx->once_code_flags.size() == 65536 &&
        memcmp(ctx->once_table.data(), table, (size_t)table_len * sizeof(double)) == 0)
        return SNPM_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));         // a previous call's expansion may still read the old table / staging copy
    ctx->once_table.assign(table, table + table_len);
    HIPCHK(ctx, hipMemcpyAsync(ctx->ws_once_table.p, ctx->once_table.data(), (size_t)table_len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ctx->once_code_flags.assign(65536, (uint8_t)8);
    ctx->once_code_abs.assign(65536, 0.0);
    for (int64_t k = 0; k < table_len; ++k) {
        const uint32_t f = once_weight_flags(table[k]);
        ctx->once_code_flags[(size_t)k] = (uint8_t)f;
        ctx->once_code_abs[(size_t)k] = (f & 4) ? 0.0 : fabs(table[k]);
    }
    return SNPM_OK;
}

struct OnceQueryGuard {     // every exit of a call frees its query (the buffers return to the context's cache); the message stays
    snpm_query *q;
    snpm_ctx *ctx;
    ~OnceQueryGuard()
    {
        const std::string keep = ctx->err;
        snpm_query_free(q);
        ctx->err = keep;
    }
};

// the pinned slab and the per-code tables of a call's gather
static int once_gather_begin(snpm_panel *p, OnceGather &g, const double *table)
{
    snpm_ctx *ctx = p->ctx;
    g.lay_out();
    int rc = ensure_pinned(ctx, std::max<size_t>(g.row_bytes + g.wei_bytes + 64, (4 * (size_t)p->n_acc + 2) * sizeof(int64_t)));
    if (rc) return rc;
    g.slab = (char *)ctx->h_pinned;
    if (g.coded() && g.n > 0) {
        if ((rc = once_set_table(ctx, table, g.table_len))) return rc;
        g.code_flags = ctx->once_code_flags.data();
        g.code_abs = ctx->once_code_abs.data();
    }
    if (g.n > 0 && g.n_wei == 0) return set_err(ctx, SNPM_ERR_BADARG, "please provide same number of positions for both sample and db");
    return SNPM_OK;
}

// what the gather refuses: the call ends before a kernel consumes the slab
static int once_refuse(snpm_ctx *ctx, const OnceGather &g, const OnceSums &s)
{
    if (s.bad_at >= 0)
        return set_err(ctx, SNPM_ERR_BADARG, "row index %lld at %lld outside the panel (n_snp %lld), or a sample index / weight code outside the weights",
                       (long long)g.row_idx[s.bad_at], (long long)s.bad_at, (long long)g.n_snp);
    if (s.flags & 4) return set_err(ctx, SNPM_ERR_BADARG, "SNP weights must be finite (a NaN or infinite weight was given)");
    return SNPM_OK;
}

// what the gather learned about the weights chooses the kernels; hard calls on a packed panel get their weight bits (reads q->d_w)
static int once_set_weight_props(snpm_panel *p, snpm_query *q, const OnceSums &s, int64_t n)
{
    snpm_ctx *ctx = p->ctx;
    q->wsum = (double)s.tot * 1.0000001;                // the same margin as the device sum of query_finish_setup
    q->all_integer = !(s.flags & 1) && s.tot < 9.0e15L;
    q->hard01 = q->all_integer && !(s.flags & 2) && p->packed;
    if (!q->hard01 || n == 0) return SNPM_OK;
    const int64_t padded = n + 16;
    hipError_t e2 = query_alloc(q, (void **)&q->d_wbits, (size_t)padded);
    if (e2 != hipSuccess) return set_err(ctx, SNPM_ERR_OOM, "query allocation failed: %s", hipGetErrorString(e2));
    hipLaunchKernelGGL(k_wbits, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)q->d_w, n, padded, q->d_wbits);
    HIPCHK(ctx, hipGetLastError());
    return SNPM_OK;
}

// h_out = {score, ninfo, lik, lrt} x n_acc, the flagged count, the status word: to the caller
static int once_read_out(snpm_ctx *ctx, const snpm_query *q, const int64_t *h_out, size_t na, double *score, int64_t *ninfo, double *lik,
                         double *lrt, int64_t *info)
{
    if (h_out[4 * na + 1] & 1) return set_err(ctx, SNPM_ERR_DOMAIN, "provided y is greater than n");       // core/snpmatch.py:43
    memcpy(score, h_out, na * sizeof(double));
    memcpy(ninfo, h_out + na, na * sizeof(int64_t));
    if (lik) {
        memcpy(lik, h_out + 2 * na, na * sizeof(double));
        memcpy(lrt, h_out + 3 * na, na * sizeof(double));
    }
    if (info) {
        const int64_t n_flag = h_out[4 * na];
        info[0] = n_flag;
        info[1] = q->all_integer ? 1 : 0;
        info[2] = n_flag > REEVAL_CAP ? 3 : (n_flag > 0 ? q->reeval_path : 0);
    }
    return SNPM_OK;
}

// ---- the fused form (default).  The slab stays in pinned host memory and k_once_prep reads it over the bus while it expands it
// (fp64 samples too: 6.4 MB per 200k SNPs read in place 0.33-0.35 ms, through the copy engine 0.37-0.38), k_fast, two reduce
// kernels, the sparse tier (its patch inside k_scan_few), k_once_finish writing into the pinned slab.  The > REEVAL_CAP tier runs
// only when the count that comes back says so (second round trip, rare).
static int genotype_once_fused(snpm_panel *p, OnceGather &g, const double *table, int64_t chunk, int skip_hets, int mode, double *score,
                               int64_t *ninfo, double *lik, double *lrt, int64_t *info)
{
    snpm_ctx *ctx = p->ctx;
    const bool coded = g.coded();
    const int64_t n = g.n, n_snp = g.n_snp;
    const size_t na = (size_t)p->n_acc;
    const int skip = skip_hets ? 1 : 0;
    OnceTrace trace;
    snpm_query *q = nullptr;
    int rc = query_alloc_all(p, n, true, &q);
    if (rc) return rc;
    OnceQueryGuard guard{q, ctx};
    q->row0 = 0;
    if ((rc = ensure(ctx, ctx->ws_once_state, 64))) return rc;
    if (!ctx->once_state_clean) {                                   // first use, or a call that failed between prep and finish
        HIPCHK(ctx, hipMemsetAsync(ctx->ws_once_state.p, 0, 64, ctx->stream));
        ctx->once_state_clean = true;
    }
    // rows per task: small enough that threads which wake late still find work (28 tasks of 7168 rows filled a 200k-SNP fp64
    // sample in 0.20 ms, 49 of 4096 in 0.13), at most ~256 tasks
    g.piece = std::max<int64_t>(4096, ((n + 255) / 256 + 1023) / 1024 * 1024);
    if ((rc = once_gather_begin(p, g, table))) return rc;
    host_pool(ctx)->run(g.n_tasks(), [&](int t) { g.fill(t); });
    trace.t_filled = OnceTrace::now();
    const OnceSums sums = g.reduce();
    if ((rc = once_refuse(ctx, g, sums))) return rc;

    // ---- prep: one launch (reads the pinned slab in place)
    void *d_slab = nullptr;
    HIPCHK(ctx, hipHostGetDevicePointer(&d_slab, g.slab, 0));
    const void *src_rows = d_slab, *src_wei = (const char *)d_slab + g.row_bytes;
    const int64_t K = (n + chunk - 1) / chunk;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(K, 2048));
    if ((rc = ensure(ctx, ctx->ws_epart, (size_t)grid * sizeof(double)))) return rc;
    ctx->once_state_clean = false;                                  // until k_once_finish has cleared the words again
    if (coded)
        hipLaunchKernelGGL((k_once_prep<true>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, src_rows, src_wei, (const double *)ctx->ws_once_table.p,
                           (int)g.table_len, n, n_snp, chunk, skip, q->d_row_idx, q->d_w, q->d_lut, (double *)ctx->ws_epart.p, q->cert_eref(),
                           q->cert_count(), (unsigned *)ctx->ws_once_state.p, (int)PREFETCH_PAD_ROWS);
    else
        hipLaunchKernelGGL((k_once_prep<false>), dim3((unsigned)grid), dim3(256), 0, ctx->stream, src_rows, src_wei, (const double *)nullptr, 0, n,
                           n_snp, chunk, skip, q->d_row_idx, q->d_w, q->d_lut, (double *)ctx->ws_epart.p, q->cert_eref(), q->cert_count(),
                           (unsigned *)ctx->ws_once_state.p, (int)PREFETCH_PAD_ROWS);
    HIPCHK(ctx, hipGetLastError());
    q->lut_skip = skip;
    q->eref_chunk = chunk;
    q->eref_after = 0;
    q->cert_count_clean = true;
    if ((rc = once_set_weight_props(p, q, sums, n))) return rc;

    // ---- score: fast pass + reduce (+ certificate), the sparse tier behind it; strict mode: the chain
    bool certified = false;
    if (mode == SNPM_MODE_STRICT) {
        q->count_valid = false;
        q->last_kernel = "k_strict4";
        if ((rc = run_strict_chain(q, skip, chunk, nullptr, nullptr, nullptr, q->d_score, q->d_ninfo))) return rc;
    } else {
        Certify cert;
        cert.on = (mode == SNPM_MODE_EXACT);
        cert.chunk = chunk;
        if ((rc = run_fast(q, skip, nullptr, cert))) return rc;
        certified = cert.on && !q->all_integer;
    }
    if ((rc = ensure(ctx, ctx->ws_lik_l, na * sizeof(double)))) return rc;
    int64_t *h_out = (int64_t *)g.slab;
    int64_t *d_out = (int64_t *)d_slab;                 // the results are written straight into the slab
    // the sparse tier behind the fast pass; its chain kernel also does the likelihood / ratio / status step (k_once_tail)
    bool tail_done = false;
    if (certified) {
        OnceTail tail;
        tail.d_ninfo = q->d_ninfo; tail.n_acc = (int64_t)na; tail.want_lik = lik ? 1 : 0;
        tail.state = (unsigned *)ctx->ws_once_state.p; tail.lik_tmp = (double *)ctx->ws_lik_l.p; tail.out = d_out;
        const bool fuse = ctx->once_tail && !single_accession(p);
        if ((rc = enqueue_reevaluation(q, skip, chunk, false, fuse ? &tail : nullptr))) return rc;
        tail_done = fuse;
    }
    auto finish = [&]() -> int {
        hipLaunchKernelGGL(k_once_finish, dim3(1), dim3(1024), 0, ctx->stream, (const double *)q->d_score, (const int64_t *)q->d_ninfo, (int64_t)na,
                           lik ? 1 : 0, certified ? (const int *)q->cert_count() : (const int *)nullptr, (unsigned *)ctx->ws_once_state.p,
                           (double *)ctx->ws_lik_l.p, d_out);
        HIPCHK(ctx, hipGetLastError());
        return SNPM_OK;
    };
    if (!tail_done && (rc = finish())) return rc;
    trace.t_enqueued = OnceTrace::now();
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->once_state_clean = true;
    if (h_out[4 * na + 1] & 6)
        return set_err(ctx, SNPM_ERR_BADARG, "a row index outside the panel (n_snp %lld), or a sample index / weight code outside the weights", (long long)n_snp);
    if (certified && h_out[4 * na] > REEVAL_CAP) {      // the dense tier, now that the count is known: everything in reference order
        if ((rc = run_strict_chain(q, skip, chunk, q->cert_count(), nullptr, nullptr, q->d_score, q->d_ninfo))) return rc;
        ctx->once_state_clean = false;
        if ((rc = finish())) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->once_state_clean = true;
    }
    trace.report(g, " (fused)");
    return once_read_out(ctx, q, h_out, na, score, ninfo, lik, lrt, info);
}

// ---- the unfused form: the slab through the copy engine, the kernels of the query path, one packed copy back
static int genotype_once_unfused(snpm_panel *p, OnceGather &g, const double *table, int64_t chunk, int skip_hets, int mode, double *score,
                                 int64_t *ninfo, double *lik, double *lrt, int64_t *info)
{
    snpm_ctx *ctx = p->ctx;
    const bool coded = g.coded();
    const int64_t n = g.n;
    const size_t na = (size_t)p->n_acc;
    snpm_query *q = nullptr;
    int rc = query_alloc_all(p, n, true, &q);
    if (rc) return rc;
    OnceQueryGuard guard{q, ctx};
    q->row0 = 0;
    g.piece = coded ? 8192 : 4096;
    if ((rc = once_gather_begin(p, g, table))) return rc;
    int32_t *d_rows32 = nullptr;
    uint16_t *d_codes = nullptr;
    if (coded && n > 0 &&
        (query_alloc(q, (void **)&d_rows32, g.row_bytes) != hipSuccess || query_alloc(q, (void **)&d_codes, g.wei_bytes) != hipSuccess))
        return set_err(ctx, SNPM_ERR_OOM, "query allocation failed");
    HostPool *pool = host_pool(ctx);
    const int n_tasks = g.n_tasks();
    OnceTrace trace;
    // The slab goes up BEHIND the fill: task 0 of the pool run is the uploader -- it waits (in order) for the fill tasks of each
    // piece and enqueues that piece's two copies, while the other threads keep filling.  Without pool threads the calling thread
    // fills everything first.  25 tasks x 4096 rows: a 200k-SNP sample goes up in two pieces (every copy costs ~25 us on its own:
    // 13 pieces 0.38 ms, 2 pieces 0.19 ms, 1 piece 0.21 ms of GPU-side wait)
    constexpr int kTasksPerPiece = 25;
    const int n_pieces = (n_tasks + kTasksPerPiece - 1) / kTasksPerPiece;
    std::vector<std::atomic<int>> piece_done((size_t)std::max(n_pieces, 1));
    for (auto &c : piece_done) c.store(0, std::memory_order_relaxed);
    std::atomic<int> upload_error{0};
    auto upload_piece = [&](int k) -> bool {
        const int64_t i0 = (int64_t)k * kTasksPerPiece * g.piece, i1 = std::min<int64_t>(n, i0 + (int64_t)kTasksPerPiece * g.piece);
        if (coded)
            return hipMemcpyAsync(d_rows32 + i0, g.rows32() + i0, (size_t)(i1 - i0) * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                   hipMemcpyAsync(d_codes + 3 * i0, g.wcodes() + 3 * i0, (size_t)(i1 - i0) * 3 * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
        return hipMemcpyAsync(q->d_row_idx + i0, g.rows() + i0, (size_t)(i1 - i0) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
               hipMemcpyAsync(q->d_w + 3 * i0, g.weights() + 3 * i0, (size_t)(i1 - i0) * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
    };
    const bool overlapped = pool->size() > 0 && n_pieces > 1;
    if (overlapped) {
        pool->run(n_tasks + 1, [&](int t) {
            if (t == 0) {                                          // the uploader
                if (hipSetDevice(ctx->device) != hipSuccess) { upload_error.store(1); return; }
                for (int k = 0; k < n_pieces; ++k) {
                    const int need = std::min(kTasksPerPiece, n_tasks - k * kTasksPerPiece);
                    while (piece_done[(size_t)k].load(std::memory_order_acquire) < need) {
#if defined(__x86_64__)
                        _mm_pause();
#endif
                    }
                    if (!upload_piece(k)) { upload_error.store(1); return; }
                }
                return;
            }
            g.fill(t - 1);
            piece_done[(size_t)((t - 1) / kTasksPerPiece)].fetch_add(1, std::memory_order_release);
        });
    } else {
        pool->run(n_tasks, [&](int t) { g.fill(t); });
    }
    trace.t_filled = OnceTrace::now();
    const OnceSums sums = g.reduce();
    if (sums.bad_at >= 0 || (sums.flags & 4) || upload_error.load()) (void)hipStreamSynchronize(ctx->stream);     // pieces already on their way read the slab
    if ((rc = once_refuse(ctx, g, sums))) return rc;
    if (upload_error.load()) return set_err(ctx, SNPM_ERR_HIP, "upload of the sample failed");
    if (!overlapped)
        for (int k = 0; k < n_pieces; ++k)
            if (!upload_piece(k)) return set_err(ctx, SNPM_ERR_HIP, "upload of the sample failed");
    if (coded && n > 0) {          // widen the row list, expand the codes: the query then looks like any other
        if ((rc = ensure(ctx, ctx->ws_flags2, 64))) return rc;
        hipLaunchKernelGGL(k_check_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, q->d_row_idx, (const int32_t *)d_rows32, n,
                           p->n_snp, (int *)ctx->ws_flags2.p);
        hipLaunchKernelGGL(k_expand_codes, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint16_t *)d_codes,
                           (const double *)ctx->ws_once_table.p, 3 * n, q->d_w);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemsetAsync(q->d_row_idx + n, 0, PREFETCH_PAD_ROWS * sizeof(int64_t), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(q->d_cert, 0, 16, ctx->stream));
    if ((rc = once_set_weight_props(p, q, sums, n))) return rc;

    // ---- the scoring pipeline of snpm_query_run_device, then the likelihoods of the truncated counts
    void *d_s = nullptr, *d_n = nullptr;
    rc = snpm_query_run_device(q, chunk, skip_hets, mode, &d_s, &d_n, nullptr);
    if (rc) return rc;
    const bool certified = (mode == SNPM_MODE_EXACT) && !q->all_integer && n > 0;
    if ((rc = ensure(ctx, ctx->ws_lik_l, na * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->ws_lik_r, na * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->ws_once, (4 * na + 2) * sizeof(int64_t)))) return rc;
    if (lik) {
        rc = snpm_likelihood_device(ctx, d_s, d_n, 1, (int64_t)na, 1, __builtin_nan(""), ctx->ws_lik_l.p, ctx->ws_lik_r.p, nullptr);
        if (rc) return rc;
    }
    // ---- one packed copy back, one synchronisation
    hipLaunchKernelGGL(k_once_pack, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)d_s,
                       (const int64_t *)d_n, lik ? (const double *)ctx->ws_lik_l.p : nullptr,
                       lik ? (const double *)ctx->ws_lik_r.p : nullptr, certified ? (const int *)q->cert_count() : nullptr,
                       lik ? (const int *)ctx->ws_flags.p : nullptr, (int64_t)na, (int64_t *)ctx->ws_once.p);
    HIPCHK(ctx, hipGetLastError());
    int64_t *h_out = (int64_t *)g.slab;                 // the inputs have left the slab by the time this copy runs (same stream)
    HIPCHK(ctx, hipMemcpyAsync(h_out, ctx->ws_once.p, (4 * na + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    trace.t_enqueued = OnceTrace::now();
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    trace.report(g, "");
    return once_read_out(ctx, q, h_out, na, score, ninfo, lik, lrt, info);
}

// codes != NULL: the sample's weights as dictionary codes, wei[r, c] = table[codes[3 r + c]] (snpm_genotype_once_coded)
static int genotype_once_impl(snpm_panel *p, const int64_t *row_idx, const double *wei, const uint16_t *codes, const double *table,
                              int64_t table_len, const int64_t *sample_idx, int64_t n_wei, int64_t n, int64_t chunk, int skip_hets,
                              int mode, double *score, int64_t *ninfo, double *lik, double *lrt, int64_t *info)
{
    CHECK_PANEL(p);
    snpm_ctx *ctx = p->ctx;
    const bool coded = codes != nullptr;
    if (coded) {
        CHECK_ARG(ctx, table != nullptr && table_len >= 1 && table_len <= 65536, "weight table of 1 .. 65536 entries expected");
        CHECK_ARG(ctx, p->n_snp < ((int64_t)1 << 31), "coded samples travel with 32-bit row indices");
    }
    CHECK_ARG(ctx, n >= 0 && n_wei >= 0, "n must be >= 0");
    CHECK_ARG(ctx, chunk >= 1, "chunk must be >= 1");
    CHECK_ARG(ctx, mode == SNPM_MODE_EXACT || mode == SNPM_MODE_STRICT || mode == SNPM_MODE_FAST, "unknown mode");
    CHECK_ARG(ctx, n == 0 || (row_idx && (wei || coded)), "please provide same number of positions for both sample and db");
    CHECK_ARG(ctx, sample_idx || n <= n_wei, "please provide same number of positions for both sample and db");
    CHECK_ARG(ctx, score && ninfo && ((lik == nullptr) == (lrt == nullptr)), "score / ninfo outputs missing, or only one likelihood output");
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = wait_upload(p);
    if (rc) return rc;
    OnceGather g{row_idx, wei, codes, table_len, sample_idx, n_wei, n, p->n_snp, 0};
    const bool fused = ctx->once_fused && n > 0 && chunk <= ONCE_MAX_CHUNK;
    return (fused ? genotype_once_fused : genotype_once_unfused)(p, g, table, chunk, skip_hets, mode, score, ninfo, lik, lrt, info);
}

int snpm_genotype_once(snpm_panel *p, const int64_t *row_idx, const double *wei, const int64_t *sample_idx, int64_t n_wei,
                       int64_t n, int64_t chunk, int skip_hets, int mode, double *score, int64_t *ninfo, double *lik,
                       double *lrt, int64_t *info)
try {
    return genotype_once_impl(p, row_idx, wei, nullptr, nullptr, 0, sample_idx, n_wei, n, chunk, skip_hets, mode, score, ninfo, lik, lrt, info);
} SNPM_GUARD((p ? p->ctx : nullptr))

// The same call with DICTIONARY-CODED weights: wei[r, c] = table[codes[3 r + c]] (codes uint16 [n_wei, 3], table fp64 [table_len]).
// A VCF sample's weights are exp(-PL / 10) of small integer PLs (core/parsers.py:141-151): the caller computes the table with its
// own libm, so the device weights carry the fp64 path's bits, and 10 instead of 32 bytes per matched SNP cross PCIe.
int snpm_genotype_once_coded(snpm_panel *p, const int64_t *row_idx, const uint16_t *codes, const double *table, int64_t table_len,
                             const int64_t *sample_idx, int64_t n_wei, int64_t n, int64_t chunk, int skip_hets, int mode,
                             double *score, int64_t *ninfo, double *lik, double *lrt, int64_t *info)
try {
    if (p && p->ctx && !codes) return set_err(p->ctx, SNPM_ERR_BADARG, "weight codes missing");
    return genotype_once_impl(p, row_idx, nullptr, codes, table, table_len, sample_idx, n_wei, n, chunk, skip_hets, mode, score, ninfo, lik,
                              lrt, info);
} SNPM_GUARD((p ? p->ctx : nullptr))
