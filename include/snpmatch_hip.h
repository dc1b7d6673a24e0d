/*
 * snpmatch_hip.h -- C ABI of libsnpmatch_hip.so, the MI355X (gfx950) scoring engine that replaces
 * the numpy hot path of SNPmatch's Genotyper / CrossIdentifier.
 *
 * Plain C, plain pointers and sizes; no C++ or torch types cross this line.  It is what a ctypes
 * binding inside the reference would call (see INTEGRATION.md for that stub).  Reference
 * interfaces replaced (paths relative to the SNPmatch v5.0.1 tree):
 *
 *   snpm_score_dense_host   <- matchGTsAccs(sampleWei, t1001snps, skip_hets_db)      core/snpmatch.py:74-89
 *   snpm_query_run          <- the chunk loop of Genotyper.genotyper                 core/snpmatch.py:207-225
 *                              (gather g.g.snps[idx,:] :222, matchGTsAccs :223, accumulate :224-225)
 *   snpm_query_run_windows  <- the window loop of CrossIdentifier.window_genotyper   core/csmatch.py:80-90
 *   snpm_likelihood         <- likeliTest + GenotyperOutput.calculate_likelihoods    core/snpmatch.py:40-55,106-117
 *   snpm_binom_identity     <- np_test_identity (binom.sf)                           core/snpmatch.py:57-72
 *   snpm_panel_*            <- HDF5Genotype.snps (int8 [num_snps,num_accessions])    pygwas/genotype.py:534-550
 *                              as an HBM-resident panel fed by a pinned-host staging path
 *
 * Conventions
 *   - every function returns int: SNPM_OK (0) or a negative SNPM_ERR_*; the message is available
 *     from snpm_last_error(ctx) (ctx == NULL: last error of a failed snpm_init in this thread).
 *   - the caller owns every host buffer it passes in (inputs are never modified) and every output
 *     buffer (pre-allocated, C-contiguous); the library owns device memory and pinned staging
 *     buffers behind the opaque handles.  No pointer handed out outlives its handle.
 *   - lifetime: free queries before their panel and panels before their context.  The other orders are
 *     tolerated: snpm_panel_free releases the device memory of the panel's live queries, snpm_destroy that of
 *     the context's live panels and queries; the orphaned handles stay valid for exactly one call, their own
 *     snpm_query_free / snpm_panel_free (a host-side delete), every other entry point refuses them with
 *     SNPM_ERR_STATE.  After the process has started to exit (exit handlers running) free / destroy only drop
 *     host bookkeeping and make no HIP call.
 *   - calls are blocking from the caller's view unless the name says otherwise; one ctx must not
 *     be used from two threads at once; distinct ctx are independent.  One ctx == one GPU; a
 *     multi-GPU job is a snpm_group (below): one process that drives every GPU, or one process per
 *     GPU, each member holding an accession range of the DB, with ONE RCCL all-gather of the
 *     per-accession results inside snpm_group_gather_scores.
 *   - genotype codes: 0 hom-ref, 1 hom-alt, 2 het, negative = missing (stored as -1);
 *     values > 2 are informative but match nothing (stored as 3).
 *   - weights `wei` are float64 [n,3]: column 0 scores db==0, column 1 scores db==2 (het),
 *     column 2 scores db==1, exactly as sampleWei in the reference.
 */
#ifndef SNPMATCH_HIP_H
#define SNPMATCH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNPM_OK            0
#define SNPM_ERR_BADARG   -1   /* argument violates the contract (the Python layer raises AssertionError) */
#define SNPM_ERR_HIP      -2   /* a HIP runtime call or kernel launch failed */
#define SNPM_ERR_OOM      -3   /* device or pinned-host allocation failed */
#define SNPM_ERR_STATE    -4   /* handle used in the wrong state */
#define SNPM_ERR_DOMAIN   -5   /* likelihood: a score exceeds its informative count (reference asserts y <= n) */
#define SNPM_ERR_RCCL     -6   /* RCCL could not be loaded, or a communicator / collective call failed */

/* scoring modes of snpm_query_run */
#define SNPM_MODE_EXACT   0    /* fast streaming pass + strict re-evaluation of every accession whose score could
                                  truncate differently from the reference: int(score) and ninfo are bit-exact,
                                  fp64 scores are within the returned error bound of the reference's */
#define SNPM_MODE_STRICT  1    /* reference summation order for every accession: fp64 scores bit-exact */
#define SNPM_MODE_FAST    2    /* fast streaming pass only (benchmarks of the dominant kernel) */

typedef struct snpm_ctx   snpm_ctx;
typedef struct snpm_panel snpm_panel;
typedef struct snpm_query snpm_query;
typedef struct snpm_carry snpm_carry;
typedef struct snpm_group snpm_group;

/* ---------------------------------------------------------------- lifecycle */
int         snpm_version(void);
/* HIP version of the build (HIP_VERSION: major * 10000000 + minor * 100000 + patch); no GPU needed */
int         snpm_hip_build_version(void);
/* 12 hex digits: hash of the sources this library was built from (build_lib.sh).  Recorded measurements (profiles/pmc_traffic.json)
   carry it; bench.py reports such a figure only for the build it was collected on. */
const char *snpm_build_id(void);
int         snpm_device_count(int *count);
int         snpm_init(int device_id, snpm_ctx **out);
int         snpm_destroy(snpm_ctx *ctx);
const char *snpm_last_error(const snpm_ctx *ctx);
/* run the library's kernels on a caller-provided hipStream_t (e.g. torch's current stream);
   NULL restores the library's own stream */
int         snpm_set_stream(snpm_ctx *ctx, void *hip_stream);
int         snpm_synchronize(snpm_ctx *ctx);
/* free / total device memory of the context's GPU in bytes (the host layer plans the residency of a DB with it: int8
   whole -> 2-bit packed whole -> SNP slabs streamed through two half-buffers) */
int         snpm_device_mem_info(snpm_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);

/* ---------------------------------------------------------------- panel (DB genotype matrix in HBM) */
/* SNP-major int8 [n_snp, pitch], pitch = n_acc rounded up to 256 B (to 128 B where that saves 5 % of the row, + 256 B where it
   would be a multiple of 8 KiB: read it with snpm_panel_info / snpm_panel_row_pitch), pad bytes = -1.  1 <= n_acc <= 2^27 (SNPM_ERR_BADARG). */
int snpm_panel_create(snpm_ctx *ctx, int64_t n_snp, int64_t n_acc, snpm_panel **out);
/* Same panel with 2 bits per call (4 accessions per byte: 0 ref, 1 alt, 2 het, 3 missing; rows either whole at a 256-B pitch or
   SPLIT -- the whole 256-B column blocks of a row in a main matrix, its ragged tail at a narrow pitch of its own -- where that saves
   5 % of the row: snpm_panel_row_pitch / snpm_panel_info report main + tail bytes per row; SNPM_PACKED_SPLIT=0 keeps whole rows): 4x less HBM
   capacity and traffic (the 10k x 50M panel is 125 GB and fits one MI355X).  Rows are uploaded as int8
   exactly like an int8 panel and packed on the device; codes > 2 cannot be stored (SNPM_ERR_BADARG from the
   upload).  Every scoring entry point accepts either panel kind and returns identical results. */
int snpm_panel_create_packed(snpm_ctx *ctx, int64_t n_snp, int64_t n_acc, snpm_panel **out);
int snpm_panel_is_packed(const snpm_panel *panel, int *packed);
/* This panel holds only some accession columns (a rank's shard) of a DB of n_acc_total accessions.  Only n_acc_total == 1
   against > 1 matters: for a panel of ONE accession numpy reduces the reference's [1, n] product along a contiguous axis, i.e.
   pairwise inside 8192-element pieces, where every wider panel is summed row after row (core/snpmatch.py:85-87) -- the
   reference-order kernels follow the rule of the width the reference would see.  Default: the panel's own n_acc. */
int snpm_panel_set_total_accessions(snpm_panel *panel, int64_t n_acc_total);
/* Bytes per row a panel of n_acc accessions will have on this context (what snpm_panel_info reports afterwards): for callers
   that size a panel to a memory budget before creating it. */
int snpm_panel_row_pitch(snpm_ctx *ctx, int64_t n_acc, int packed, int64_t *pitch);
int snpm_panel_free(snpm_panel *panel);
int snpm_panel_info(const snpm_panel *panel, int64_t *n_snp, int64_t *n_acc, int64_t *pitch, void **device_ptr);
/* Asynchronous upload of rows [row0, row0+nrows) from host memory (row stride host_pitch bytes,
   >= n_acc): rows are copied into double-buffered pinned staging slabs, sent with hipMemcpyAsync on a side
   stream and written into the panel by a device kernel (the panel's row pitch, codes canonicalised:
   negative -> -1, >2 -> 3; 2-bit packing for packed panels).
   Returns once the last slab is enqueued; scoring calls wait for it on the device. */
int snpm_panel_upload_rows(snpm_panel *panel, int64_t row0, int64_t nrows, const int8_t *host, int64_t host_pitch);
/* Same pipeline fed from a file of tightly packed int8 rows (n_acc bytes per row) that starts at byte
   file_offset (the data section of snps.npy in a native flat panel): pread() straight into the pinned slabs. */
int snpm_panel_load_file(snpm_panel *panel, const char *path, int64_t file_offset, int64_t row0, int64_t nrows);
/* The general file form: the file holds an int8 matrix with file_pitch bytes per row (>= col0 + n_acc) from byte
   file_offset on; panel row row0 + i receives columns [col0, col0 + n_acc) of file row row_idx[i] (row_idx != NULL: the
   matched rows of a sample, the reference's g.g.snps[idx, :], core/snpmatch.py:222) or file_row0 + i.  col0 / file_pitch
   serve an accession shard of a wider DB.  Contiguous reads of >= 1 GiB use O_DIRECT where the file system takes it
   (SNPM_ODIRECT=0/1 overrides); packed panels are packed to 2 bits per call by the host threads that fill the slabs
   (SNPM_HOST_PACK=0: on the device), so a quarter of the bytes cross PCIe. */
int snpm_panel_load_file_rows(snpm_panel *panel, const char *path, int64_t file_offset, int64_t file_pitch, int64_t col0,
                              const int64_t *row_idx, int64_t file_row0, int64_t row0, int64_t nrows);
/* The same from a PACKED flat file (2 bits per call, 4 accessions per byte as in a packed panel; file_pitch = BYTES per file
   row): accessions [acc0, acc0 + n_acc) (acc0 a multiple of 4) of file row row_idx[i] or file_row0 + i.  Either panel kind
   takes it (an int8 panel is unpacked on the device); a quarter of the bytes leave the disk and cross PCIe. */
int snpm_panel_load_file_rows_packed(snpm_panel *panel, const char *path, int64_t file_offset, int64_t file_pitch, int64_t acc0,
                                     const int64_t *row_idx, int64_t file_row0, int64_t row0, int64_t nrows);
/* the loader's host-side packer on its own (no ctx, no GPU): int8 calls [nrows, n_acc] (row stride src_pitch) -> 2 bits
   per call, (n_acc + 3) / 4 bytes per row (row stride dst_pitch; field f of byte b = call 4 b + f: 0 ref, 1 alt, 2 het,
   3 missing = any negative; fields past n_acc are 3).  *bad (may be NULL) = 1 when a call > 2 was met. */
int snpm_pack_rows_host(const int8_t *src, int64_t src_pitch, int64_t nrows, int64_t n_acc, uint8_t *dst, int64_t dst_pitch,
                        int force_scalar, int *bad);
int snpm_panel_upload_wait(snpm_panel *panel);
int snpm_panel_download_rows(snpm_panel *panel, int64_t row0, int64_t nrows, int8_t *host, int64_t host_pitch);
/* Device-side synthetic fill (benchmarks; no PCIe): element (snp, acc) is a pure function of
   (seed, snp0 + row, acc0 + col) with P(-1,0,1,2) = (3277, 39321, 21627, 1311)/65536.
   snpmatch_amd.synth.panel_values() is the numpy twin used by the tests. */
int snpm_panel_fill_synthetic(snpm_panel *panel, uint64_t seed, int64_t snp0, int64_t acc0);
/* the same for panel rows [row0, row0 + nrows) only: row r receives SNP snp0 + (r - row0) of the synthetic panel
   (slab-streamed benchmarks refill a resident buffer with the next SNP slab) */
int snpm_panel_fill_synthetic_rows(snpm_panel *panel, uint64_t seed, int64_t snp0, int64_t acc0, int64_t row0, int64_t nrows);
/* Device-side synthetic sample for benchmarks (the recipe of SURVEY 8d, no host pass over the SNP axis): rows
   [snp0, snp0 + n) of accession `planted` of the synthetic panel `seed`, with a fraction err_permille / 1000 of the
   calls replaced at random; pl_permille / 1000 of the rows get PL-derived weights exp(-PL/10) (integer PL 1..255, 0
   for the called genotype), the others hard 0/1 weights.  d_wei: DEVICE float64 [n, 3].  exp_table: HOST float64
   [256], exp_table[k] = exp(-k / 10) as the caller's libm rounds it (so that a host twin reproduces the bits);
   snpmatch_amd.synth.sample_weights_twin() is that twin. */
int snpm_sample_synthetic(snpm_ctx *ctx, uint64_t seed, int64_t snp0, int64_t n, int64_t planted, int err_permille,
                          int pl_permille, const double *exp_table, void *d_wei);

/* ---------------------------------------------------------------- query (one sample's matched SNPs, resident) */
/* row_idx: int64 [n] panel rows matched by the sample (commonSNPs[0]); NULL = the dense range
   [row0, row0+n).  wei: float64 [n,3] = inputs.wei[commonSNPs[1]].  Both are copied to the device. */
int snpm_query_create(snpm_panel *panel, const int64_t *row_idx, int64_t row0, int64_t n,
                      const double *wei, snpm_query **out);
/* The same query from DEVICE arrays (int64 row list or NULL, float64 [n,3] weights); both are copied.  The row
   indices are not read back: the caller guarantees that they lie inside the panel. */
int snpm_query_create_device(snpm_panel *panel, const void *d_row_idx, int64_t row0, int64_t n, const void *d_wei,
                             snpm_query **out);
int snpm_query_free(snpm_query *query);

/* Genotyper.genotyper over the whole matched list with `chunk`-row matchGTsAccs calls (1000 in the
   reference).  Outputs (host pointers, may be NULL): score float64 [n_acc] (ScoreList before the int
   truncation), ninfo int64 [n_acc].  info (may be NULL), int64 [4]:
   [0] accessions re-evaluated in strict order, [1] 1 if all weights are integers (any order exact),
   [2] how they were re-read (1 accession-major copy, 2 SNP-major strided, 3 every accession: more than 64 flagged);
   the bound itself via snpm_query_error_bound.
   SNPM_MODE_EXACT never waits for the certificate on the host: the accessions the fast pass cannot vouch for
   are flagged by the last reduce kernel, and the re-evaluation kernels queued behind it read that list on the
   device (asking for `info` costs one synchronisation).  */
int snpm_query_run(snpm_query *query, int64_t chunk, int skip_hets, int mode,
                   double *score, int64_t *ninfo, int64_t *info);
/* Same, leaving results in device memory (pointers owned by the query, valid until the next run /
   free): d_score float64 [n_acc], d_ninfo int64 [n_acc].  Work is enqueued on the ctx stream. */
int snpm_query_run_device(snpm_query *query, int64_t chunk, int skip_hets, int mode,
                          void **d_score, void **d_ninfo, int64_t *info);
/* number of accessions the last certified run re-evaluated (synchronises), name of its scoring kernel */
int snpm_query_last_reeval(snpm_query *query, int64_t *n_flagged);
const char *snpm_query_last_kernel(const snpm_query *query);
/* Redirect the results of subsequent runs into caller-owned DEVICE buffers (e.g. torch tensors that
   feed an RCCL all-gather): d_score float64 [n_acc], d_ninfo int64 [n_acc].  NULL, NULL restores the
   query's own buffers. */
int snpm_query_bind_outputs(snpm_query *query, void *d_score, void *d_ninfo);
/* Rigorous bound on |fast-pass score - reference score| used by SNPM_MODE_EXACT for this query. */
int snpm_query_error_bound(snpm_query *query, int64_t chunk, double *bound);

/* CrossIdentifier.window_genotyper: one matchGTsAccs call per window w over matched rows
   [win_off[w], win_off[w+1]) (reference order, fp64 bit-exact).  Outputs (host, may be NULL):
   score float64 [n_win, n_acc], ninfo int64 [n_win, n_acc], totals accumulated window after
   window: tot_score float64 [n_acc], tot_ninfo int64 [n_acc]. */
int snpm_query_run_windows(snpm_query *query, const int64_t *win_off, int64_t n_win, int skip_hets,
                           double *score, int64_t *ninfo, double *tot_score, int64_t *tot_ninfo);

/* The same for one SNP slab of a DB scored slab after slab (slabs hold whole windows): the totals continue in `carry`
   (reference order: the fp64 bits of one pass over all windows; read them with snpm_carry_finish).  The call does NOT
   wait for the device: score / ninfo [n_win, n_acc] should be pinned host memory (snpm_host_alloc) and are complete when
   snpm_carry_finish or snpm_synchronize returns -- the caller loads the next slab meanwhile. */
int snpm_query_run_windows_carry(snpm_query *query, const int64_t *win_off, int64_t n_win, int skip_hets, double *score,
                                 int64_t *ninfo, snpm_carry *carry);

/* The same window loop at streaming speed (one segmented fast pass over all windows + the certificate per
   (window, accession) and for the totals; uncertain entries are re-scored in reference order): int(score), ninfo and
   the totals' counts are bit-exact, fp64 window scores agree with the reference's to ~1e-12 relative (likelihoods
   well inside the 1e-6 of north_star).  snpm_query_run_windows above is the byte-identical mode.
   info (may be NULL) int64 [4]: [0] (window, accession) pairs re-scored, [1] totals re-scored, [2] 1 = fell back to
   the strict pass (more uncertain entries than the sparse tiers take). */
int snpm_query_run_windows_fast(snpm_query *query, const int64_t *win_off, int64_t n_win, int skip_hets,
                                double *score, int64_t *ninfo, double *tot_score, int64_t *tot_ninfo, int64_t *info);

/* ---------------------------------------------------------------- many samples per call */
/* ONE sample against a resident panel in ONE call: Genotyper.genotyper (core/snpmatch.py:207-241: gather of the matched weight rows
   :221, chunk loop :218-225) followed by GenotyperOutput's truncation and likelihoods (:96, :106-117).  row_idx [n]: matched DB rows;
   wei [n_wei, 3]: the sample's weights; sample_idx [n] (or NULL = rows 0..n-1): row of wei for each matched SNP -- the library's host
   threads gather wei[sample_idx] straight into a pinned slab, check the indices and derive the weight properties on the way (no
   device pass, no read-back), the slab goes up, LUT / fast pass / reduce + certificate / gated reference-order tiers / likelihood
   are enqueued back to back, and score, ninfo, lik, lrt [n_acc each] (lik / lrt of the TRUNCATED counts; both NULL = skip) return
   in one copy after one synchronisation.  mode / chunk / skip_hets as snpm_query_run; info (may be NULL) as there.
   SNPM_ERR_BADARG (-> AssertionError) for indices outside the panel / the weights and non-finite weights, SNPM_ERR_DOMAIN when a
   count exceeds its informative sites (the reference's assert, :43). */
int snpm_genotype_once(snpm_panel *panel, const int64_t *row_idx, const double *wei, const int64_t *sample_idx, int64_t n_wei,
                       int64_t n, int64_t chunk, int skip_hets, int mode, double *score, int64_t *ninfo, double *lik,
                       double *lrt, int64_t *info);
/* The same call with DICTIONARY-CODED weights: wei[r, c] = table[codes[3 r + c]], codes uint16 [n_wei, 3], table fp64 [table_len <= 65536]
   (as snpm_score_batch_coded).  A VCF sample's weights are exp(-PL / 10) of small integer PLs (core/parsers.py:141-151): the caller
   computes the table with its own libm, so the device weights carry the fp64 path's bits; the matched rows travel as 32-bit
   indices (n_snp < 2^31), 10 instead of 32 bytes per matched SNP cross PCIe.  A code >= table_len is SNPM_ERR_BADARG. */
int snpm_genotype_once_coded(snpm_panel *panel, const int64_t *row_idx, const uint16_t *codes, const double *table, int64_t table_len,
                             const int64_t *sample_idx, int64_t n_wei, int64_t n, int64_t chunk, int skip_hets, int mode,
                             double *score, int64_t *ninfo, double *lik, double *lrt, int64_t *info);

/* B samples against one resident panel.  The reference scores one sample per process (core/snpmatch.py:256-268); here
   sample b owns entries [sample_off[b], sample_off[b+1]) of the concatenated row list (int64, panel rows matched by the
   sample = commonSNPs[0]) and weights (float64 [N,3] = inputs.wei[commonSNPs[1]]); device_inputs != 0: both are DEVICE
   pointers.  One launch scores all samples (sample on the grid), the certificate runs per (sample, accession) on the
   device, likelihood rows [B, n_acc] come from one launch (scores truncated first, as GenotyperOutput does), results
   return in one copy.  Outputs (host, may be NULL; lik and lrt both or neither): score / ninfo / lik / lrt [B, n_acc].
   mode as snpm_query_run: EXACT = int(score) and ninfo bit-exact per sample.
   info (may be NULL) int64 [4]: [0] (sample, accession) pairs re-scored in reference order, [1] 1 = every sample went
   through the strict pass (more uncertain pairs than the sparse tier takes), [2] 1 = scored by the shared-row pass
   (snpm_batch_configure below), [3] its union rows. */
int snpm_score_batch(snpm_panel *panel, int64_t n_samples, const int64_t *sample_off, const void *row_idx, const void *wei,
                     int device_inputs, int64_t chunk, int skip_hets, int mode, double *score, int64_t *ninfo,
                     double *lik, double *lrt, int64_t *info);

/* The same with dictionary-coded weights, wei[r, c] = table[codes[r, c]] (codes uint16 [N, 3], table float64
   [table_len <= 65536], host; codes >= table_len read 0.0): for samples whose weights are exp(-PL/10) of integer PLs
   (core/parsers.py:141-151) the caller fills the table with its own libm, the device weights then carry the bits the
   fp64 path would have received, and 6 + 4 instead of 24 + 8 bytes per matched SNP cross PCIe (the link bounds a batch
   from host memory). */
int snpm_score_batch_coded(snpm_panel *panel, int64_t n_samples, const int64_t *sample_off, const int64_t *row_idx,
                           const uint16_t *codes, const double *table, int64_t table_len, int64_t chunk, int skip_hets,
                           int mode, double *score, int64_t *ninfo, double *lik, double *lrt, int64_t *info);

/* Batches whose samples SHARE DB rows (many samples genotyped on largely the same markers, the production use of the reference:
   one `snpmatch inbred` process per sample over the same panel, core/snpmatch.py:218-225 per sample): instead of one gathered pass
   per sample, the union of the batch's matched rows is formed on the device, every DB row is read ONCE and scored against all
   samples as an int8 MFMA contraction -- the weights as fixed-point numbers of `digits` base-256 digits (w in [0, 1] ->
   floor(w 2^F), F = 8 (digits - 1) + 6), the panel rows as one-hot class bytes, products added exactly in int32.  The pass has
   no rounding error, only the one-sided quantisation n_inexact 2^-F per sample; the certificate of SNPM_MODE_EXACT covers it and
   the unproven (sample, accession) pairs are re-scored in reference order as before: int(score) and ninfo stay bit-exact.
   Taken when every sample's row list is strictly increasing, all weights lie in [0, 1] and the panel holds no call code > 2;
   otherwise (and in SNPM_MODE_STRICT) the per-sample pass runs.  The weights are vetted while they are converted, i.e. after
   the pass was taken: a batch with a weight outside [0, 1] is scored AGAIN through the per-sample pass inside the same call
   (results as if the shared-row pass had never run; stats [1] = 4, info[2] = 0).
     shared_rows  -1 (default; SNPM_BATCH_SHARED) automatic: batches whose inputs are already on the device (device_inputs != 0),
                  of at least 4 samples, with at least min_density calls per (sample, union row) slot;  0 never;
                  1 whenever the batch allows it (host batches are uploaded whole first)
     digits       3..7, or -1 (default; SNPM_SHARED_DIGITS=0): the fewest digits that keep a sample's quantisation below 2^-20 --
                  5 up to 262 144 matched SNPs per sample, 6 up to 2^26, else 7; 0 keeps the current value
     min_density  threshold of the automatic choice (default 0.11 on int8, 0.21 on packed panels, 0.5 for fewer than 8 samples; SNPM_SHARED_MIN_DENSITY); negative keeps the current value
   snpm_score_batch[_coded] report in info[2] whether the shared-row pass scored the batch and in info[3] its union rows. */
int snpm_batch_configure(snpm_ctx *ctx, int shared_rows, int digits, double min_density);
/* stats int64 [8] of the context's last snpm_score_batch[_coded] call: [0] 1 = shared-row pass taken, [1] else why not (1 policy,
   2 too few samples or rows, 3 a row list not strictly increasing, 4 a weight outside [0, 1], 5 call codes > 2 in the panel,
   6 overlap below min_density, 7 sizes beyond 32-bit indices or more than 65 535 samples, 8 a row index outside the panel), [2] union rows, [3] density * 1e6, [4] row tiles, [5] groups of
   128 matrix rows, [6] passes over groups, [7] digits */
int snpm_batch_last_stats(snpm_ctx *ctx, int64_t *stats);

/* pinned host memory (hipHostMalloc): batch inputs built in it go to the device at full PCIe speed without the
   staging copy (snpm_score_batch recognises pinned pointers) */
int snpm_host_alloc(snpm_ctx *ctx, int64_t bytes, void **out);
int snpm_host_free(snpm_ctx *ctx, void *ptr);

/* ---------------------------------------------------------------- jobs larger than HBM: SNP slab after SNP slab */
/* The reference walks the whole SNP axis in `chunk`-row pieces and adds every piece onto ScoreList / NumInfoSites
   (core/snpmatch.py:218-225).  When the panel does not fit in HBM the caller loads (or regenerates) one SNP slab
   after the other into a resident panel, makes a query of the slab's rows and weights, and scores it with a
   snpm_carry that holds the running totals:
     STRICT  the chain of additions continues across slabs: fp64 bits of the reference over the whole job;
     EXACT / FAST  fast pass per slab, totals added in slab order; the error bounds of the slabs add up
             (every addition of the reference's chain is charged in the slab where it happens, by the magnitude
             the totals of the slabs scored so far allow; chunks_after = number of `chunk`-row pieces in the slabs
             still to come: non-zero says that this slab is not the last one and must end on a chunk boundary)
             and snpm_carry_finish certifies the TOTALS: it returns the accessions whose int(score) is not
             yet proven.  For those the caller streams the slabs once more through a second, column-list carry
             (snpm_carry_set_columns + snpm_query_run_carry in STRICT mode) and patches the result in
             (snpm_carry_patch); more than 64 flagged: a second pass in STRICT mode over all accessions.
   Every slab but the last must hold a multiple of `chunk` rows.  snpmatch_amd.engine.SlabScorer drives this. */
int snpm_carry_create(snpm_ctx *ctx, int64_t n_acc, snpm_carry **out);
int snpm_carry_reset(snpm_carry *carry);
int snpm_carry_free(snpm_carry *carry);
/* keep the totals in caller-owned DEVICE buffers (float64 [n_acc], int64 [n_acc]); resets the carry */
int snpm_carry_bind_outputs(snpm_carry *carry, void *d_score, void *d_ninfo);
int snpm_carry_set_columns(snpm_carry *carry, const int32_t *cols, int64_t ncols);
int snpm_query_run_carry(snpm_query *query, int64_t chunk, int skip_hets, int mode, int64_t chunks_after,
                         snpm_carry *carry);
/* score / ninfo (host, may be NULL): the totals; flagged [cap] / n_flagged: see above (0 unless EXACT) */
int snpm_carry_finish(snpm_carry *carry, double *score, int64_t *ninfo, int32_t *flagged, int64_t cap,
                      int64_t *n_flagged);
int snpm_carry_patch(snpm_carry *totals, const snpm_carry *cols_pass);
/* Rigorous bound on |total - reference total| of the slabs scored so far in SNPM_MODE_EXACT (the sum of the slabs'
   bounds -- reference-order term of every slab, integer-weight slabs included, plus the fast-pass term of the
   non-integer ones -- and of the slab-order additions); 0 when every slab had integer weights or in other modes. */
int snpm_carry_error_bound(snpm_carry *carry, double *bound);
/* device pointers of the totals (float64 [n_acc], int64 [n_acc]): input of snpm_likelihood_device / an all-gather */
int snpm_carry_device_ptrs(snpm_carry *carry, void **d_score, void **d_ninfo);

/* ---------------------------------------------------------------- multi-GPU: accession shards + one RCCL all-gather */
/* Every reduction of matchGTsAccs runs over SNPs (core/snpmatch.py:84-88): accession columns never interact, so
   member r of a group of R GPUs holds columns [a0_r, a1_r) of every SNP row (snpm_group_shard; boundaries are
   multiples of 4 accessions), scores them with the entry points above on its own context, and the only exchange is
   the gather of (score float64, ninfo int64) per accession -- the likelihood step needs the minimum over ALL
   accessions (core/snpmatch.py:112).  Two ways to form a group:
     snpm_group_create_local   ONE process drives n GPUs (ncclCommInitAll, no launcher): the group creates the n
                               contexts (snpm_group_ctx) and destroys them with snpm_group_free;
     snpm_group_create_rank    one process per GPU: rank 0 calls snpm_group_unique_id, hands the 128 bytes to the
                               other ranks by any channel (file, environment, socket), every rank then joins with
                               its own context (ncclCommInitRank).
   RCCL is bound at the first group call (dlopen: the copy already in the process, else the one beside the HIP
   runtime in use, else librccl.so.1; SNPMATCH_RCCL_LIB overrides); SNPM_ERR_RCCL when none loads.
   Errors of group calls: snpm_group_last_error(group) (group == NULL: last failed creation in this thread). */
#define SNPM_GROUP_ID_BYTES 128
#define SNPM_GROUP_LOOPBACK 1   /* snpm_group_create_local flag: exchange by device-to-device copies instead of RCCL; a TEST
                                   transport (it also accepts one device several times: rehearsal on a one-GPU box) */
int snpm_group_unique_id(void *id_bytes /* [SNPM_GROUP_ID_BYTES] */);
int snpm_group_create_rank(snpm_ctx *ctx, const void *id_bytes, int world, int rank, snpm_group **out);
int snpm_group_create_local(const int *device_ids, int n, int flags, snpm_group **out);
int snpm_group_free(snpm_group *group);
const char *snpm_group_last_error(const snpm_group *group);
/* world = ranks of the job, rank0 = global rank of local member 0, n_local = members this process drives */
int snpm_group_info(const snpm_group *group, int *world, int *rank0, int *n_local);
int snpm_group_ctx(snpm_group *group, int member, snpm_ctx **ctx);
/* accession range [a0, a1) of global rank `rank` in a DB of n_acc accessions (equal shards of ceil(n_acc / world)
   rounded up to 4; the last ranks may be short or empty) */
int snpm_group_shard(const snpm_group *group, int64_t n_acc, int rank, int64_t *a0, int64_t *a1);
/* The collective.  d_score[i] / d_ninfo[i] (i < n_local): DEVICE results of local member i's shard, float64 / int64
   [m, a1_i - a0_i] with row stride in_ld elements (m = 1: genome-wide totals, e.g. the pointers of
   snpm_query_run_device / snpm_carry_device_ptrs; m = n_win: window rows), produced by work queued on that member's
   stream.  Per member one pack kernel, ONE ncclAllGather (16 * m * per bytes per rank) and one unpack kernel run on
   that stream; with lik / lrt the likelihood rows over all accessions follow on member 0 (`truncate` as in
   snpm_likelihood).  Host outputs [m, n_acc] (any may be NULL; lik and lrt both or neither) come from member 0 and
   the call waits for them; with every host output NULL nothing waits on the host.  Every rank of the job makes the
   same call (same m, n_acc). */
int snpm_group_gather_scores(snpm_group *group, const void *const *d_score, const void *const *d_ninfo, int64_t m,
                             int64_t n_acc, int64_t in_ld, int truncate, double *score, int64_t *ninfo, double *lik,
                             double *lrt);
/* device arrays the last gather left on a local member: float64 / int64 [m, n_acc] (valid until the next gather) */
int snpm_group_gathered_ptrs(snpm_group *group, int member, void **d_score_all, void **d_ninfo_all);
/* path of the RCCL library in use, or "loopback" */
const char *snpm_group_transport(const snpm_group *group);

/* ---------------------------------------------------------------- one-shot forms */
/* matchGTsAccs on host arrays: db int8 [n, n_acc] (row stride db_pitch), wei float64 [n,3].
   fp64 bit-exact with the reference (strict order). */
int snpm_score_dense_host(snpm_ctx *ctx, const int8_t *db, int64_t db_pitch, int64_t n, int64_t n_acc,
                          const double *wei, int skip_hets, double *score, int64_t *ninfo);

/* likeliTest over rows: y float64 [m, len] (matches; truncated toward zero first when
   truncate != 0, as GenotyperOutput does for inbred), n int64 [m, len].  Per row r:
   lik[r,:] = likeliTest, lrt[r,:] = lik / nanmin(lik[r,:]) (amin_or_nan: use this TopHit
   instead when it is not NaN).  Host pointers.  SNPM_ERR_DOMAIN if some y > n. */
int snpm_likelihood(snpm_ctx *ctx, const double *y, const int64_t *n, int64_t m, int64_t len,
                    int truncate, double amin_or_nan, double *lik, double *lrt);
/* device-pointer form used after snpm_query_run_device (m = 1) */
int snpm_likelihood_device(snpm_ctx *ctx, const void *d_y, const void *d_n, int64_t m, int64_t len,
                           int truncate, double amin_or_nan, void *d_lik, void *d_lrt, int *domain_error);

/* np_test_identity on the device: out[i] = (binom.sf((n[i]-x[i]) - 1, n[i], error_rate) >= pthres).  Host
   pointers; sf (may be NULL) receives the survival function values. */
int snpm_binom_identity(snpm_ctx *ctx, const double *x, const int64_t *n, int64_t len, double error_rate,
                        double pthres, int64_t *out, double *sf);
/* host twin of the device arithmetic of snpm_binom_identity: sf[i] = binom.sf(k[i], n[i], p) (no ctx, no GPU) */
int snpm_binom_sf_host(const double *k, const double *n, int64_t len, double p, double *sf);

/* ---------------------------------------------------------------- caller-side index preparation */
/* Sorted-merge intersection of two strictly increasing int64 arrays (the positions of one chromosome in the
   DB and in the sample): ia / ib receive the indices of the common values (capacity min(na, nb)), *n_out
   their number.  Replaces the two np.in1d calls per chromosome of Genotype.get_common_positions
   (core/snp_genotype.py:66-67).  Pure host code, needs no ctx / GPU.  SNPM_ERR_STATE when an input is not
   strictly increasing (the caller then takes its generic path). */
int snpm_intersect_sorted(const int64_t *a, int64_t na, const int64_t *b, int64_t nb, int64_t *ia, int64_t *ib,
                          int64_t *n_out);
/* Same result for a short list b against a long list a: galloping search, O(nb log(na / nb)); from 4096 values of b on the search
   runs in ranges of b on a pool of host threads.  Capacity of ia / ib: min(na, nb), as above.  a must be
   strictly increasing and is NOT checked here (DB positions are verified once, when the DB is opened);
   b is checked (SNPM_ERR_STATE). */
int snpm_intersect_sorted_search(const int64_t *a, int64_t na, const int64_t *b, int64_t nb, int64_t *ia, int64_t *ib,
                                 int64_t *n_out);
/* Genotype.identify_segregating_snps on the resident panel (core/snp_genotype.py:188-211, used by --refine):
   mask [n_snp] (host, uint8) = 1 where the informative calls of accessions cols[0..ncols) are not all equal. */
int snpm_panel_segregating(snpm_panel *panel, const int32_t *cols, int64_t ncols, uint8_t *mask);
/* the same scan for an accession-SHARDED DB (ncols may be 0): besides the local mask, first [n_snp] receives the
   first informative call of the listed local accessions in every row (0xFF = none); a row segregates when some
   rank's mask is set or two ranks report different calls (snpmatch_amd.dist) */
int snpm_panel_segregating_first(snpm_panel *panel, const int32_t *cols, int64_t ncols, uint8_t *mask, uint8_t *first);
/* calls of the listed accessions at the query's matched rows, codes [ncols, n] (uint8: 0 ref, 1 alt, 2 het, 3 other
   code, 0xFF missing; host): the g_acc.snps[:, i] column reads of the reference (core/csmatch.py:116-117), used to
   bring the columns of an accession-sharded DB together for the in-silico crosses */
int snpm_query_gather_columns(snpm_query *query, const int32_t *acc_idx, int ncols, uint8_t *codes);
/* CrossIdentifier.match_insilico_f1s (core/csmatch.py:115-125): every pair (i < j, in the order of
   itertools.combinations) of the n_sel (<= 32) accessions acc_idx is crossed in silico over the query's
   matched SNPs.  Per pair: "alt" SNPs (both calls 1) take W[:, 2], "ref" SNPs (both 0) take W[:, 0], SNPs
   where both calls are informative and differ take W[:, 1];
       score = (np.sum(alt weights) + np.sum(ref weights)) + np.sum(het weights),  ninfo = the three counts.
   The reference prints these scores as floats, so each np.sum is evaluated in numpy's order (pairwise
   summation inside 8192-element chunks, chunks added in sequence): fp64 bit patterns of the reference.
   score / ninfo: host arrays [n_sel * (n_sel - 1) / 2].  DB codes other than -1, 0, 1, 2 count as one
   further class (differs from 0/1/2, equal to itself). */
int snpm_query_f1_pairs(snpm_query *query, const int32_t *acc_idx, int n_sel, double *score, int64_t *ninfo);

/* ---------------------------------------------------------------- profiling (HIP events on the ctx stream) */
/* PMC calibration: reads the whole panel once with the access shape of the scoring kernel (4 B per
   lane, non-temporal); *bytes_read = n_snp * pitch.  Used by tools/pmc_traffic.py to calibrate
   FETCH_SIZE on a known byte count. */
int snpm_debug_stream_read(snpm_panel *panel, int64_t *bytes_read);
int snpm_profile_enable(snpm_ctx *ctx, int on);
int snpm_profile_reset(snpm_ctx *ctx);
/* kernel: "fast", "strict", "reduce", "scan", "likelihood", "synth", "lut", "gcross", "ghmm", "pairs_t" (transpose of
   snpm_pair_counts), "pairs_c" (its count), "kin_planes" / "kin_count" (the two kernels of snpm_panel_kinship_counts),
   "site_counts" (the kernel of snpm_panel_site_counts, one launch per slab), "ld_planes" / "ld_band" (the two kernels of
   snpm_panel_ld_band, one launch each per slab), "win_planes" / "win_count" (the two kernels of snpm_panel_window_counts, one
   launch each per slab), "f1x_count" (the count kernel of snpm_panel_f1_counts, one launch per slab; its planes are a
   "win_planes" launch per slab), "par_count" (the count kernel of snpm_panel_parent_counts, one launch per slab of whole windows
   and 65535 groups; its planes are a "win_planes" launch per slab), "sim_noise" / "sim_count" (the two kernels of
   snpm_panel_sim_counts, one launch each per slab, "sim_noise" only with err_thr > 0; its planes are a "win_planes" launch per
   slab), "mos_fwd" / "mos_back" (the two kernels of snpm_panel_mosaic, one launch each per slab of whole chains and group of
   samples; its planes are a "win_planes" launch per slab), "ibd_count" / "ibd_runs" (the two kernels of snpm_panel_ibd_counts:
   "ibd_count" one launch per slab of whole windows and 65535 groups, "ibd_runs" one launch per call; its planes are a "win_planes"
   launch per slab), "mk_planes" / "mk_gain" / "mk_pick" / "mk_update" (the four kernels of snpm_panel_marker_select: "mk_planes"
   one launch per call, "mk_gain" and "mk_pick" one per enqueued round, "mk_update" one per enqueued round and one more for the
   initial need; rounds are enqueued eight at a time, so up to seven of them behind the end of the loop return at once),
   "pca_gram" / "pca_fold" (the two kernels of snpm_panel_gram, one launch each per slab; its planes are a "win_planes" launch per
   slab), "pca_load" (the kernel of snpm_panel_loadings, one launch per slab), "adm_rows" / "adm_cols" / "adm_fold" (the three
   kernels of snpm_panel_admix: "adm_rows" and "adm_fold" one launch per iteration, "adm_cols" one per iteration with
   SNPM_ADMIX_UPDATE_Q), "mix_count" (the count kernel of snpm_panel_mix_counts, one launch per slab; its planes are a
   "win_planes" launch per slab).
   Synchronises the stream. */
int snpm_profile_read(snpm_ctx *ctx, const char *kernel, int64_t *launches, double *total_ms);

/* ---------------------------------------------------------------- genotype_cross */
/* GenotypeCross.genotype_cross (core/genotype_cross.py:210-241 of the reference: a Python loop over windows x samples around
   getWindowGenotype, :21-49) as ONE device call.  Host pointers in and out.
     gt_codes [n, ld]  call codes (as snpm_vcf_parse_calls produces them) of every sample at the n matched segregating markers,
                       markers in window order, the samples of a marker contiguous, ld >= n_samples
     p1, p2 [n]        the two parents' calls (0 / 1 / 2, different at every marker)
     win_off [n_win+1] marker range of every window: 0 = win_off[0] <= ... <= win_off[n_win] = n
   Per (window, sample): the governing separator is the one of the window's FIRST marker of that sample (parseGT, core/parsers.py:
   12-35); an element's value is {0, 1, 2, -1, 0}[class] under that separator and 0 under the other one; m1 = #(value == p1),
   mh = #(value == 2), m2 = #(value == p2), tot = markers of the window; the decision is getWindowGenotype's (fp64 likeliTest).
     geno [n_win, n_samples]        -1 'NA', 0 parent 1, 1 heterozygous, 2 parent 2
     counts [n_win, n_samples, 3]   m1, mh, m2 (exact int32); NULL to skip
   Every argument is validated on the host before the context or the device is touched (SNPM_ERR_BADARG with a message; with ctx ==
   NULL the message is in snpm_last_error(NULL)); n == 0, n_win == 0 or n_samples == 0 return without a launch. */
int snpm_cross_calls(snpm_ctx *ctx, const uint8_t *gt_codes, int64_t n, int n_samples, int64_t ld, const int8_t *p1, const int8_t *p2,
                     const int64_t *win_off, int n_win, double lr_thres, int n_marker_thres, int8_t *geno, int32_t *counts);

/* ---------------------------------------------------------------- genotype_cross_hmm */
/* GenotypeCross.genotype_cross_hmm (core/genotype_cross.py:113-181 of the reference: a Python loop over chromosomes x samples around
   infer.viterbi, core/infer.py:17-58) as ONE device call: the 3-state path (0 AA, 1 AB, 2 BB) of every (chain, sample).  A chain
   is the markers of one chromosome.  Host pointers in and out.
     gt_codes [n, ld]     call codes (as snpm_vcf_parse_calls produces them), markers chain by chain, the samples contiguous
     depth_rank [n, ld]   index of rint(depth) of every call among the n_depth distinct values the tables were built for
     pair [n]             the ordered parental pair of every marker: 0 (0,1)  1 (0,2)  2 (1,0)  3 (1,2)  4 (2,0)  5 (2,1)
     chain_off [n_chain+1] marker range of every chain: 0 = chain_off[0] <= ... <= chain_off[n_chain] = n
     logT [n_chain][3][3] log of the transition matrix of every chain, [from][to]
     logI, logE [6][n_depth][4][3]   log(initial x emission) and log(emission) per (pair, depth rank, observation, state)
   Per (chain, sample): the governing separator is the one of the chain's FIRST marker of that sample; the observation of an
   element is {0, 2, 1, 3, 0}[class] under that separator and 0 under the other one.  omega[first] = logI[...];
   omega[r][j] = max over i of ((omega[r-1][i] + logT[i][j]) + logE[...][j]) with the FIRST maximum over i = 0, 1, 2 kept as
   the backpointer; the last state is the first maximum of the last omega.  Additions and comparisons in fp64 only: the tables
   carry every logarithm, -inf entries included.
     state [n, n_samples]       the path
     omega [n, n_samples, 3]    every step's omega; NULL to skip
   Every argument is validated on the host before the context or the device is touched (SNPM_ERR_BADARG with a message; with ctx ==
   NULL the message is in snpm_last_error(NULL)): chain_off from 0 to n without a decrease, ld >= n_samples, pair < 6, depth_rank <
   n_depth, defined codes only, no NaN (or +inf) in a table, no negative size.  n == 0, n_chain == 0 or n_samples == 0 return
   without a launch; an empty chain between two others reads nothing. */
int snpm_cross_hmm(snpm_ctx *ctx, const uint8_t *gt_codes, const uint16_t *depth_rank, int64_t n, int n_samples, int64_t ld,
                   const uint8_t *pair, const int64_t *chain_off, int n_chain, const double *logT, const double *logI,
                   const double *logE, int n_depth, int8_t *state, double *omega);

/* ---------------------------------------------------------------- pairsnp */
/* snpmatch.pairwiseScore (core/snpmatch.py:270-309 of the reference: two sample files, a Python loop over chromosomes) for EVERY
   pair of a set of samples as ONE device call.  Host pointers in and out.
     ids [n, ld]        one byte per (record, sample), the samples of a record contiguous, ld >= n_samples: 0 = the sample has no
                        call at this record, 1..127 = the id of its genotype text (equal texts, equal ids)
     seg_off [n_seg+1]  record range of every segment (a chromosome): 0 = seg_off[0] <= ... <= seg_off[n_seg] = n
     common [n_seg, n_samples, n_samples]   common[s][a][b] = records r of segment s with ids[r][a] != 0 && ids[r][b] != 0
     match  [n_seg, n_samples, n_samples]   match[s][a][b]  = records r of segment s with ids[r][a] == ids[r][b] != 0
   Both are full symmetric matrices of exact int32 counts; the diagonal of either is the number of calls of the sample in the
   segment.  Limits: n_samples <= SNPM_PAIR_MAX_SAMPLES, n_seg * n_samples^2 <= SNPM_PAIR_MAX_CELLS (512 MiB per result matrix), a
   segment of 2^31 records or more is refused (its counts would not fit).
   Every argument is validated on the host before the context or the device is touched (SNPM_ERR_BADARG with a message; with ctx ==
   NULL the message is in snpm_last_error(NULL)): seg_off from 0 to n without a decrease, ld >= n_samples, every id inside the
   first n_samples columns <= 127 (padding columns are not looked at and never reach the device), no negative size, the limits.
   n_seg == 0 or n_samples == 0 return without a launch and write nothing; n == 0 with n_seg > 0 writes zeros without a launch. */
#define SNPM_PAIR_MAX_SAMPLES 4096
#define SNPM_PAIR_MAX_CELLS ((int64_t)1 << 27)
int snpm_pair_counts(snpm_ctx *ctx, const uint8_t *ids, int64_t n, int n_samples, int64_t ld, const int64_t *seg_off, int n_seg,
                     int32_t *common, int32_t *match);

/* ---------------------------------------------------------------- panel kinship */
/* Genotype.kinship_given_snps / calc_kinship_mat (core/snp_genotype.py:256-289, :440-459 of the reference: a Python loop over
   1000-row chunks, two dense float products each) on the RESIDENT panel (int8 or packed), as one call.  Host pointers in and out.
     cols [ncols]     accession columns of the panel, any order, repeats allowed (a repeat counts as listed); NULL = all
                      accessions in panel order, ncols must then be the panel's accession count (or 0)
     row_idx [n_rows] panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows) (row0 is ignored
                      when row_idx is given)
     ninfo [ncols, ncols]   rows where both calls are not missing (hets and an int8 panel's "other" code included)
     same  [ncols, ncols]   rows where both calls are homozygous (0 or 1) and equal
     diff  [ncols, ncols]   rows where both calls are homozygous and different
   All three are full symmetric matrices of exact int32 counts, the diagonal included; the reference's kinship is
   (same - diff) / ninfo.  The row axis is processed in slabs whose bit-planes fit a workspace budget (512 MiB; SNPM_KIN_WS_MB,
   read by snpm_init); the counts accumulate on the device.  Limits: ncols <= SNPM_KIN_MAX_ACCESSIONS (each result matrix stays
   below 2^27 cells and the tile pairs of the count kernel below 2^16), n_rows < 2^31 (the counts are int32).
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message): no negative size, the limits, non-NULL
   outputs when ncols > 0 -- these before the panel handle is looked at, the message of a NULL panel is in snpm_last_error(NULL)
   -- then every column and row index inside the panel.  ncols == 0 returns without a launch and writes nothing; n_rows == 0
   writes zeros without a launch.  Uploads into the panel that are still in flight are waited for on the device. */
#define SNPM_KIN_MAX_ACCESSIONS 11552
int snpm_panel_kinship_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                              int32_t *ninfo, int32_t *same, int32_t *diff);

/* ---------------------------------------------------------------- site statistics */
/* Genotype.get_af_snps / calculate_af_snp_mat / _polarize_snps (core/snp_genotype.py:119-175, :360-376, :385-394 of the
   reference: a Python loop over 1000-row chunks that gathers the panel again for every subpopulation) on the RESIDENT panel (int8
   or packed), as one call that reads every selected row once for all groups.  Host pointers in and out.
     cols, grp_off    CSR lists of accession columns: group g = cols[grp_off[g] .. grp_off[g + 1]), grp_off [n_groups + 1] starts at
                      0 and does not decrease; a group may be empty, groups may overlap, a column may be listed ONCE per group
                      (engine.site_counts splits a list with repeats into layers).  cols == NULL and grp_off == NULL with
                      n_groups == 1: one group of all accessions
     row_idx [n_rows] panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows) (row0 is ignored
                      when row_idx is given)
     counts [n_groups][n_rows][4]   per group and row: c0, c1, c2 = members with canonical code 0 (ref), 1 (alt), 2 (het); ninfo =
                      members whose call is not missing.  An int8 panel's "other" code 3 is informative and in none of c0..c2
   The row axis is processed in slabs whose counts fit a workspace budget (256 MiB; SNPM_SITE_WS_MB, read by snpm_init):
   slab_rows = max(64, floor(budget / (16 * n_groups)) rounded down to a multiple of 64), one launch per slab.
   Limits: n_groups <= SNPM_SITE_MAX_GROUPS (the membership words of a launch are held in the 64 KiB of LDS of a block), panels
   of at most 16384 accessions (eight 32-column words per lane of a wave).
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size,
   n_groups within the limit, grp_off starts at 0 and does not decrease, non-NULL counts when there is work -- these before the
   panel handle is looked at, the message of a NULL panel is in snpm_last_error(NULL) -- then every column inside the panel, no
   column twice in one group, every row inside the panel.  n_groups == 0 or n_rows == 0 returns without a launch and writes
   nothing; a call whose groups are all empty writes zeros without a launch.  Uploads into the panel that are still in flight
   are waited for on the device. */
#define SNPM_SITE_MAX_GROUPS 32
int snpm_panel_site_counts(snpm_panel *panel, const int32_t *cols, const int64_t *grp_off, int64_t n_groups, const int64_t *row_idx,
                           int64_t row0, int64_t n_rows, int32_t *counts);

/* ---------------------------------------------------------------- panel LD */
/* Genotype.calculate_ld / calculate_ld (core/snp_genotype.py:291-295, :348-358 of the reference; neither runs there) on the
   RESIDENT panel (int8 or packed): linkage disequilibrium of every selected row with each of the `band` rows after it, as one call.
   Host pointers in and out.
     cols [ncols]     distinct accession columns, any order; NULL = all accessions (ncols is ignored then)
     row_idx [n_rows] panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows) (row0 is ignored when
                      row_idx is given).  Row k of the SELECTION is paired with rows k + 1 .. k + band of the selection
     counts [n_rows][band][9]   per row k and offset d = 1 .. band (j = k + d), over the selected columns, with a = canonical code 1
                      (alt), h = code 2 (het), m = code 0, 1 or 2 (an int8 panel's "other" code 3 and missing calls are outside m):
                      n = |m_k & m_j|, Ak = |a_k & m_j|, Hk = |h_k & m_j|, Aj = |a_j & m_k|, Hj = |h_j & m_k|, AA = |a_k & a_j|,
                      AH = |a_k & h_j|, HA = |h_k & a_j|, HH = |h_k & h_j|.  NULL = not wanted
     r2 [n_rows][band]   squared Pearson correlation of the two rows' genotype values (v_alt for code 1, v_het for code 2, 0 for
                      code 0; both 0 .. 3) over the n common columns, from exact integers:
                        sx = v_alt Ak + v_het Hk, sxx = v_alt^2 Ak + v_het^2 Hk, sy / syy alike from Aj, Hj,
                        sxy = v_alt^2 AA + v_alt v_het (AH + HA) + v_het^2 HH,
                        num = n sxy - sx sy, dx = n sxx - sx^2, dy = n syy - sy^2   (int64),
                        r2 = (double(num) * double(num)) / (double(dx) * double(dy))
                      -- three correctly rounded operations, the same bits on every machine, never above 1.  NaN where n < min_n
                      (min_n >= 1), where dx or dy is 0 (a row constant among the common columns).  NULL = not wanted
   Cells with k + d >= n_rows hold zeros / NaN.  Every cell is written exactly once.
   The row axis is processed in slabs whose planes (12 bytes per 32 columns and row, the `band` halo rows behind the slab included)
   and outputs (44 bytes per cell) fit a workspace budget (256 MiB; SNPM_LD_WS_MB, read by snpm_init); a slab is a multiple of 64
   rows, at least 64; two launches per slab.
   Limits: panels of at most 16384 accessions; band <= SNPM_LD_MAX_BAND, which bounds what the smallest slab of 64 rows takes on the
   device whatever the budget: 64 x 4096 cells x 44 bytes = 11 MiB of outputs and 64 + 4096 plane rows (25 MiB at 16384 accessions).
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size,
   band, v_alt, v_het and min_n in range, not both outputs NULL when there is work -- these before the panel handle is looked at,
   the message of a NULL panel is in snpm_last_error(NULL) -- then every column inside the panel, no column twice, every row inside
   the panel, the panel's width.  n_rows == 0 returns without a launch and writes nothing.  Uploads into the panel that are still
   in flight are waited for on the device. */
#define SNPM_LD_MAX_BAND 4096
int snpm_panel_ld_band(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                       int64_t band, int32_t v_alt, int32_t v_het, int32_t min_n, int32_t *counts, double *r2);
/* Greedy marker pruning on a band of r2 values (host only, no context, no GPU), in row order: keep[k] = 1 when row k is eligible
   (eligible == NULL: every row) and no KEPT row j in [k - band, k) has r2[j][k - j - 1] > threshold; else 0.  NaN never prunes.
   r2 [n_rows][band] as snpm_panel_ld_band writes it; eligible, keep [n_rows] bytes.  SNPM_ERR_BADARG for a negative n_rows,
   band < 1, or a NULL r2 / keep with n_rows > 0. */
int snpm_ld_prune(int64_t n_rows, int64_t band, const double *r2, const uint8_t *eligible, double threshold, uint8_t *keep);

/* ---------------------------------------------------------------- panel windows */
/* Genotype.calculate_heterozygosity_windows / mismatch_between_accs (core/snp_genotype.py:297-345 of the reference) on the RESIDENT
   panel (int8 or packed): per genome window the call counts of every listed accession column and the agreement counts of listed
   pairs of columns, as one call.  Host pointers in and out.
     cols [ncols]      accession columns, any order, repeats allowed; NULL = all accessions (ncols must then be the panel's count)
     pair_a, pair_b [n_pairs]   pair i is columns cols[pair_a[i]] and cols[pair_b[i]]: indices INTO THE COLUMN LIST, 0 .. ncols - 1;
                       a == b is allowed, (a, b) and (b, a) are both allowed
     row_idx [n_rows]  panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows)
     win_off [n_win + 1]   offsets into the SELECTED rows: starts at 0, never decreases, ends at n_rows; window w holds the selected
                       rows [win_off[w], win_off[w + 1]).  Empty windows are allowed anywhere
     acc_counts [n_win][ncols][4]   c0, c1, c2 = rows of the window with canonical code 0 / 1 / 2 in that column, ninfo = rows whose
                       call is not missing (an int8 panel's "other" code 3 counts in ninfo and in none of c0 .. c2; negative int8
                       values and the 2-bit value 3 are missing).  NULL = not wanted
     pair_counts [n_pairs][n_win][4]   n = rows where both calls are 0, 1 or 2; eq = rows among those where the two codes are equal
                       (het against het is equal); hom_same / hom_diff = rows where both are homozygous and equal / different
                       (summed over the windows: same / diff of snpm_panel_kinship_counts).  NULL = not wanted
   Integers only: het = c2 / ninfo and mismatch = 1 - eq / n are the caller's (snp_genotype.het_from_counts / mismatch_from_counts).
   The selected rows are processed in slabs: accession-major bit-planes (4 bits per call, whole steps of 1024 rows, at least one)
   plus the cells of the slab's windows fit a workspace budget (256 MiB; SNPM_WIN_WS_MB, read by snpm_init); two launches per slab,
   its cells are added into the zeroed outputs on the host, so the result does not depend on the budget.
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size,
   win_off sound, not both outputs NULL when there is work, pair_a / pair_b given with n_pairs > 0, n_rows < 2^31,
   ncols <= SNPM_WIN_MAX_ACCESSIONS (the grid of the plane kernel) -- these before the panel handle is looked at, the message of a
   NULL panel is in snpm_last_error(NULL) -- then every column inside the panel, every pair index inside the column list, every row
   inside the panel.  n_win == 0 or ncols == 0 writes nothing; n_rows == 0 writes zeros without a launch.  Uploads into the panel
   that are still in flight are waited for on the device. */
#define SNPM_WIN_MAX_ACCESSIONS 4194240
int snpm_panel_window_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs,
                             const int64_t *row_idx, int64_t row0, int64_t n_rows, const int64_t *win_off, int64_t n_win, int32_t *acc_counts,
                             int32_t *pair_counts);

/* ---------------------------------------------------------------- f1search */
/* The in-silico F1 of EVERY pair of listed accession columns scored against one sample's hard calls over panel rows -- the
   exhaustive form of CrossIdentifier.match_insilico_f1s (core/csmatch.py:106-129 of the reference, which crosses the ten best single
   accessions only: snpm_query_f1_pairs) -- on the RESIDENT panel (int8 or packed), as one call.  Host pointers in and out.
     cols [ncols]     accession columns, any order, repeats allowed; NULL = all accessions (ncols must then be the panel's count)
     row_idx [n_rows] panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows)
     sample_class [n_rows]   the sample's class at every selected row: 0 ref, 1 alt, 2 het, 0xFF no class
   The F1 of columns a, b at a row follows the rules of snpm_query_f1_pairs on canonical DB codes (0, 1, 2, 3 = an int8 panel's
   "other" code, missing): ref when both are 0, alt when both are 1, het when both are not missing and the codes differ,
   uninformative otherwise (a call missing, 2 with 2, 3 with 3).
     ninfo [ncols, ncols]   rows where the F1 is ref, alt or het (rows of class 0xFF included)
     hits  [ncols, ncols]   rows where the F1's class is the sample's class
   Both are full symmetric matrices of exact int32 counts; the diagonal is the cross of a column with itself.  With the one-hot
   weights of a hard-called sample (ParseInputs.get_wei_from_GT) hits[a][b] IS the reference's score of the pair and ninfo its
   numinfo.  The row axis is processed in slabs whose bit-planes (4 bits per call) fit a workspace budget (512 MiB; SNPM_F1X_WS_MB,
   read by snpm_init); two launches per slab, the counts accumulate on the device, so the result does not depend on the budget.
   Limits: ncols <= SNPM_F1X_MAX_ACCESSIONS (each result matrix stays below 2^27 cells and the tile pairs of the count kernel below
   2^16), n_rows < 2^31 (the counts are int32).
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size, the
   limits, non-NULL outputs when ncols > 0, non-NULL sample_class when n_rows > 0, every class byte 0, 1, 2 or 0xFF -- these before
   the panel handle is looked at, the message of a NULL panel is in snpm_last_error(NULL) -- then every column and row inside the
   panel, then ncols == the panel's accession count when cols is NULL.  ncols == 0 writes nothing; n_rows == 0 writes zeros without
   a launch.  Uploads into the panel that are still in flight are waited for on the device. */
#define SNPM_F1X_MAX_ACCESSIONS 11552
int snpm_panel_f1_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                         const uint8_t *sample_class, int32_t *hits, int32_t *ninfo);

/* ---------------------------------------------------------------- parentsearch */
/* EVERY pair of listed accession columns scored, genome window by genome window, as the two parents of a RECOMBINANT sample (an F2,
   a backcross, a RIL with residual heterozygosity: in one stretch of the genome parent A, in the next the F1 of A and B, in the next
   parent B) against the sample's hard calls, on the RESIDENT panel (int8 or packed), as one call.  Host pointers in and out.
     cols, row_idx / row0 / n_rows, sample_class   as for snpm_panel_f1_counts
     win_off [n_win + 1]   offsets into the SELECTED rows: starts at 0, never decreases, ends at n_rows; window w holds the selected
                       rows [win_off[w], win_off[w + 1]).  Empty windows are allowed anywhere; a window may start and end anywhere
     min_win_sites     a window is used for a cell only with this many rows or more (>= 1)
   Per cell (a, b) -- positions in the column list -- and window, over the rows where the F1 of a and b is informative (the rule of
   snpm_panel_f1_counts) AND the sample has a class: n = those rows, hA / hB = rows among them where a's / b's canonical code is the
   sample's class (0 / 1 / 2; code 3 never), hF = rows where the F1's class is the sample's class.  A window with n < min_win_sites
   adds nothing to the cell.  Otherwise, with hom = max(hA, hB): if hF > hom the window is taken as the F1 (score += hF, w_het += 1),
   else as a parent (score += hom; the window counts in w_first[a][b] when hA > hB, or hA == hB and a <= b, and in w_first[b][a]
   otherwise); n_tot += n.
     score, n_tot, w_first, w_het [ncols, ncols]   exact int32.  score, n_tot and w_het are symmetric; for a != b
                       w_first[a][b] + w_first[b][a] + w_het[a][b] is the number of windows used for the pair; on the diagonal
                       w_het is 0 and w_first the number of used windows.
   The windows are processed in slabs of WHOLE windows whose bit-planes (4 bits per call) fit a workspace budget (512 MiB;
   SNPM_PAR_WS_MB, read by snpm_init; a window larger than the budget is a slab of its own); the counts accumulate on the device, so
   the result does not depend on the budget.  The host folds the window boundaries into a stream of masked 64-row segments (32
   bytes per segment, at most one per 64 rows plus one per window).  Limits: those of snpm_panel_f1_counts.
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size,
   n_win >= 0, min_win_sites >= 1, the limits, win_off sound, non-NULL outputs when ncols > 0, non-NULL sample_class when n_rows > 0,
   every class byte 0, 1, 2 or 0xFF -- these before the panel handle is looked at, the message of a NULL panel is in
   snpm_last_error(NULL) -- then every column and row inside the panel, then ncols == the panel's accession count when cols is NULL.
   ncols == 0 writes nothing; n_rows == 0 writes zeros without a launch.  Uploads into the panel that are still in flight are waited
   for on the device. */
int snpm_panel_parent_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                             const uint8_t *sample_class, const int64_t *win_off, int64_t n_win, int32_t min_win_sites, int32_t *score,
                             int32_t *n_tot, int32_t *w_first, int32_t *w_het);

/* ---------------------------------------------------------------- power */
/* The sample SIMULATED from every listed accession column -- its calls at the selected rows with call errors injected -- scored
   against every listed accession column, per group of selected rows: what simulateSNPs followed by inbred answers for one accession
   and one marker count at a time (core/simulate.py:26-53, core/snpmatch.py:74-117 of the reference), for all accessions and a whole
   ladder of marker counts, on the RESIDENT panel (int8 or packed), as one call.  Host pointers in and out.
     cols [ncols]     accession columns, any order, repeats allowed; NULL = all accessions (ncols must then be the panel's count)
     row_idx [n_rows] panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows)
     grp_off [n_grp + 1]   offsets into the SELECTED rows: starts at 0, never decreases, ends at n_rows; group g holds the selected
                      rows [grp_off[g], grp_off[g + 1]).  Empty groups are allowed anywhere; a group may start and end anywhere
     err_thr          0 .. 2^32: the call error rate times 2^32
     seed             of the counter-based hash
   On canonical DB codes (0, 1, 2, 3 = an int8 panel's "other" code, missing), with a the POSITION of a column in the column list and
   k the POSITION of a row in the selected rows: the sample of a has a call at k when a's code there is 0, 1 or 2.  Its class is that
   code unless (h >> 32) < err_thr; then it is ((h & 0xFFFFFFFF) * 3) >> 32 (which may be the code itself), with
     h = mix(mix(seed + 0x9E3779B97F4A7C15 * (a + 1)) ^ k),   mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
                                                                       z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31
   in 64-bit unsigned arithmetic (two rounds of the splitmix64 finaliser).  A column listed twice gives two independent samples.
     ninfo [n_grp][ncols][ncols]   ninfo[g][a][b] = rows of g where sample a has a call and b's code is not missing (code 3 counts)
     score [n_grp][ncols][ncols]   score[g][a][b] = rows of g where b's code is sample a's class
   Exact int32 counts; the matrices are NOT symmetric (a is the sample, b the DB column).  With the one-hot weights of the sample
   they are the reference's NumInfoSites / ScoreList.  The counts of disjoint groups add: the cumulative sum over g of a ladder of
   nested marker sets drawn by the host gives every level from one call.
   The row axis is processed in slabs whose SEVEN bit-planes (7 bits per call: four of the DB, three of the samples) fit a workspace
   budget (512 MiB; SNPM_SIM_WS_MB, read by snpm_init); up to three launches per slab, the counts accumulate on the device, and the
   hash is keyed by the position in the selection, so the result does not depend on the budget.
   Limits: ncols <= SNPM_SIM_MAX_ACCESSIONS, n_rows < 2^31, 1 <= n_grp <= 64, n_grp * ncols * ncols < 2^31.
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size, the
   limits, grp_off sound, err_thr <= 2^32, non-NULL outputs when ncols > 0 -- these before the panel handle is looked at, the
   message of a NULL panel is in snpm_last_error(NULL) -- then every column and row inside the panel, then ncols == the panel's
   accession count when cols is NULL.  ncols == 0 writes nothing; n_rows == 0 writes zeros without a launch.  Uploads into the panel
   that are still in flight are waited for on the device. */
#define SNPM_SIM_MAX_ACCESSIONS 11552
int snpm_panel_sim_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                          const int64_t *grp_off, int64_t n_grp, uint64_t err_thr, uint64_t seed, int32_t *score, int32_t *ninfo);

/* ---------------------------------------------------------------- mosaic */
/* A sample as a MOSAIC of the listed accession columns: the copying-model Viterbi (Li & Stephens with a uniform switch cost) whose
   states are all the listed columns, with integer costs, for every (chain, sample) in one call on the RESIDENT panel (int8 or
   packed).  The reference has nothing like it: inbred assumes one accession, cross two.  Host pointers in and out.
     cols [ncols]     accession columns, any order, repeats allowed; NULL = all accessions (ncols must then be the panel's count)
     row_idx [n_rows] panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows)
     chain_off [n_chain + 1]  offsets into the SELECTED rows: starts at 0, never decreases, ends at n_rows.  A chain (a chromosome)
                      is the selected rows [chain_off[c], chain_off[c + 1]); empty chains are allowed anywhere
     sample_class [n_samples][n_rows]  per sample and selected row 0 ref, 1 alt, 2 het, 0xFF no class (as snpm_panel_f1_counts)
     cost [3][4]      uint8, every entry 0 .. 15: cost[sample class][canonical DB code 0, 1, 2, 3]; 3 is an int8 panel's "other" code
     switch_cost      S, 1 .. 2^20
   With a the POSITION of a column in the column list and k the POSITION of a row in the selected rows:
     e(a, k) = cost[class of the sample at k][code of a at k]; 0 when the sample has no class at k or the call of a is missing
               (a negative int8, the 2-bit value 3); an int8 panel's code 3 is NOT missing
   and per (sample, non-empty chain [c0, c1)):
     V(a, c0) = e(a, c0);  for k > c0:  B = min_a V(a, k - 1),  j(k - 1) = the LOWEST a that attains B,
                                        sw(a, k) = V(a, k - 1) > B + S  (strict: a tie stays),
                                        V(a, k) = min(V(a, k - 1), B + S) + e(a, k)
     chain_cost = min_a V(a, c1 - 1);  state[c1 - 1] = the LOWEST a that attains it;  state[k - 1] = sw(state[k], k) ? j(k - 1) : state[k]
   A column listed twice is two states; the tie rules decide between them.
     state [n_samples][n_rows]            int32 positions in the column list
     chain_cost [n_samples][n_chain]      int32, 0 for an empty chain
     col_cost [n_samples][n_chain][ncols] int32 sum over the chain of e(a, k): the cost of never switching; NULL to skip
   The chain axis is processed in slabs of WHOLE chains whose bit-planes fit a workspace budget (512 MiB; SNPM_MOS_WS_MB, read by
   snpm_init) beside the backpointer words of one sample -- a chain larger than the budget is a slab of its own -- and the samples in
   groups of as many as fit; a chain is always computed whole by one block, so the result does not depend on the budget.
   Limits: ncols <= SNPM_MOS_MAX_ACCESSIONS, n_rows < 2^31, n_chain <= SNPM_MOS_MAX_CHAINS, 15 * (longest chain) + S < 2^31.
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size, the
   limits, chain_off sound, n_samples >= 1 when there are rows and columns, cost entries <= 15, S in range, the class bytes,
   non-NULL state / chain_cost when they would be written -- these before the panel handle is looked at, the message of a NULL
   panel is in snpm_last_error(NULL) -- then every column and row inside the panel, then ncols == the panel's accession count when
   cols is NULL.  ncols == 0 or n_samples == 0 writes nothing; n_rows == 0 writes zero costs without a launch.  Uploads into the
   panel that are still in flight are waited for on the device. */
#define SNPM_MOS_MAX_ACCESSIONS 12288
#define SNPM_MOS_MAX_CHAINS 1048576
int snpm_panel_mosaic(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                      const int64_t *chain_off, int64_t n_chain, const uint8_t *sample_class, int64_t n_samples, const uint8_t *cost,
                      int32_t switch_cost, int32_t *state, int32_t *chain_cost, int32_t *col_cost);

/* ---------------------------------------------------------------- ibd */
/* For EVERY pair of listed accession columns, WHERE along the genome the two are identical -- shared haplotype segments, identity by
   descent -- on the RESIDENT panel (int8 or packed), as one call: snpm_panel_kinship_counts counts every pair over all rows,
   snpm_panel_window_counts looks along the genome for listed pairs only.  Host pointers in and out.
     cols, row_idx / row0 / n_rows, win_off / n_win   as for snpm_panel_parent_counts (without the sample)
     min_win_sites     a window is USED for a cell only with this many rows or more (>= 1)
     max_diff_ppm      0 .. 1 000 000: the share of differing rows, in parts per million, up to which a used window is SHARED
     min_run           a run is REPORTED with this many shared windows or more (>= 1)
   Per cell (a, b) -- positions in the column list -- and window, on canonical codes: n = rows where both calls are homozygous (code
   0 or 1), d = rows among them where the two codes differ (hom_same + hom_diff and hom_diff of snpm_panel_window_counts).  Hets, an
   int8 panel's code 3 and missing calls count nowhere.  The window is used iff n >= min_win_sites, shared iff used and
   d * 1 000 000 <= max_diff_ppm * n (64-bit integers), a break iff used and not shared.  The windows of the call are scanned in
   order (a caller hands over one chromosome per call): a run is a maximal set of shared windows with no break between two
   consecutive members; unused windows neither break a run nor count in it; its length is its number of shared windows.
     w_used, w_shared  [ncols, ncols]  windows used / shared
     n_shared, d_shared [ncols, ncols] sums of n / d over the shared windows
     run_max           [ncols, ncols]  the longest run (0: none), whatever min_run
     n_runs, w_in_runs [ncols, ncols]  the reported runs and the shared windows inside them
     used_bits, shared_bits [ncols, ncols, wwords]  uint32, wwords = ceil(n_win / 32): window w is bit w % 32 of word w / 32, bits at
                       and above n_win are zero; either pointer may be NULL (that bitset is not copied back)
   Exact int32, full and symmetric; on the diagonal d = 0, so every used window is shared.
   The windows are processed in slabs of WHOLE windows whose bit-planes (4 bits per call) fit a workspace budget (512 MiB;
   SNPM_IBD_WS_MB, read by snpm_init; a window larger than the budget is a slab of its own); every (cell, window) is evaluated
   whole by one block, so the result does not depend on the budget.  The two bitsets live on the device for the whole call (the
   runs are made from them) and must fit SNPM_IBD_BITS_MB (2048 MiB, read by snpm_init; 1135 accessions x 399 windows take 134 MB):
   a call whose bitsets do not fit is refused with SNPM_ERR_BADARG, the message states the bytes needed and names the variable.
   Limits: ncols <= SNPM_F1X_MAX_ACCESSIONS, n_rows < 2^31.
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size,
   n_win >= 0, min_win_sites >= 1, max_diff_ppm in range, min_run >= 1, the limits, win_off sound, the seven matrices non-NULL when
   ncols > 0 -- these before the panel handle is looked at, the message of a NULL panel is in snpm_last_error(NULL) -- then every
   column and row inside the panel, then ncols == the panel's accession count when cols is NULL, then the bitset budget.
   ncols == 0 writes nothing; n_rows == 0 or n_win == 0 writes zeros without a launch.  Uploads into the panel that are still in
   flight are waited for on the device. */
int snpm_panel_ibd_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                          const int64_t *win_off, int64_t n_win, int32_t min_win_sites, int32_t max_diff_ppm, int32_t min_run,
                          int32_t *w_used, int32_t *w_shared, int32_t *n_shared, int32_t *d_shared,
                          int32_t *run_max, int32_t *n_runs, int32_t *w_in_runs, uint32_t *used_bits, uint32_t *shared_bits);

/* ---------------------------------------------------------------- markers */
/* A small set of panel rows (SNPs) that SEPARATES every pair of listed accession columns -- the list to genotype (an amplicon or
   KASP panel) so that no two accessions are confused -- chosen greedily on the RESIDENT panel (int8 or packed), all rounds inside
   one call.  Host pointers in and out.
     cols, row_idx / row0 / n_rows   as for snpm_panel_kinship_counts (repeats allowed; two equal columns are a pair nothing
                       separates); a POSITION below is an index into this row selection, 0 .. n_rows - 1
     coord, min_dist   coord [n_rows] int64 in any order, or NULL: a pick at position p makes every row r with
                       |coord[r] - coord[p]| < min_dist ineligible (unlinked markers); min_dist >= 0, and 0 when coord is NULL
     eligible          [n_rows] uint8, or NULL (every row): a row with eligible[r] == 0 is never picked
     depth             1 .. 255: how many chosen rows must separate every pair
     max_markers       picks at most (>= 0)
   On canonical codes, row r separates the unordered pair {a, b}, a != b, when both calls are homozygous and different (code 0 in one
   column, 1 in the other); a het, a missing call and an int8 panel's code 3 never separate.  need [ncols, ncols] (uint8, symmetric)
   starts at depth off the diagonal and 0 on it; remaining is its sum over a < b.  A round: stop with reason 0 if remaining == 0,
   else with reason 1 if n_chosen == max_markers; gain[r] = the pairs with need > 0 that eligible row r separates; stop with reason 2
   if no row is eligible or the best gain is 0; pick the eligible row with the largest gain, on a tie the smallest position; record
   it; decrement need[a][b] and need[b][a] of every pair it separates whose need is > 0; subtract the gain from remaining; the pick
   (and its neighbourhood, see coord) becomes ineligible.  This is the textbook greedy set (multi-)cover: NOT optimal -- a smaller
   set may exist.  What it guarantees: every pair that the eligible rows can separate depth times ends at need 0 unless max_markers
   stopped the loop, and with reason 2 the cells with need > 0 are exactly the pairs the candidates cannot tell apart (depth times).
   All integer: the result is one bit pattern.
     chosen, gain_at   [max_markers] int64 / int32: positions of the picks in order and their gains; entries at and above n_chosen are
                       not written (at most min(max_markers, n_rows) are); may be NULL when that bound is 0
     n_chosen, remaining  one int64 each;  stop_reason  one int32: 0 all resolved, 1 max_markers reached, 2 no eligible row with gain
     need              [ncols, ncols] uint8: the final need matrix
     first_gain        [n_rows] int32, or NULL: the gain of round 0 of EVERY row whatever its eligibility -- the pairs the SNP
                       separates
   The bit-planes of all selected rows (2 bits per call) stay on the device for the whole loop -- there are no slabs: a slab walk
   per round would read the panel again every round -- and must fit a workspace budget (1024 MiB; SNPM_MK_WS_MB, read by snpm_init):
   a call whose n_rows * 2 * ceil(ncols / 64) * 8 bytes do not fit is refused with SNPM_ERR_BADARG, the message states both figures
   and advises thinning the candidates.  Limits: ncols <= SNPM_MK_MAX_ACCESSIONS, n_rows < 2^31.
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size, depth
   in 1 .. 255, min_dist >= 0 and 0 without coord, the limits, the output pointers -- these before the panel handle is looked at, the
   message of a NULL panel is in snpm_last_error(NULL) -- then every column and row inside the panel (ncols == the panel's accession
   count when cols is NULL), then the workspace budget.  Group and streamed panels have no snpm_panel handle of this kind: the
   Python layer refuses them.  ncols < 2, n_rows == 0 or max_markers == 0 launch nothing and write the initial state: need, n_chosen
   0, remaining, the stop reason by the rules above, first_gain zeros.  Uploads into the panel that are still in flight are waited
   for on the device. */
#define SNPM_MK_MAX_ACCESSIONS 4096
int snpm_panel_marker_select(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                             const int64_t *coord, int64_t min_dist, const uint8_t *eligible, int32_t depth, int64_t max_markers,
                             int64_t *chosen, int32_t *gain_at, int64_t *n_chosen, int64_t *remaining, int32_t *stop_reason, uint8_t *need,
                             int32_t *first_gain);

/* ---------------------------------------------------------------- pca */
/* The two device primitives of a principal component analysis of the RESIDENT panel (int8 or packed): the weighted Gram matrix of
   the accession columns over panel rows -- the genotype relationship matrix before its division by the row count -- and the
   row-streaming product that turns eigenvectors into SNP loadings.  The package's own: the reference has no counterpart (its
   calc_kinship_mat is the count form, snpm_panel_kinship_counts).  Host pointers in and out.
     cols, row_idx / row0 / n_rows   as for snpm_panel_kinship_counts (cols == NULL: all accessions; repeats count as listed)
     tab [n_rows][4]   the CLASS TABLE, fp64: for selected row s the value of an accession whose canonical code is 0 (ref), 1 (alt),
                       2 (het), 3 (an int8 panel's "other" code; a packed panel has no such code).  A missing call has value 0,
                       always.  Write t(s, i) = tab[s][code(s, i)], or 0 where missing.
   snpm_panel_gram:      gram[i][j] = sum over selected rows s of t(s, i) * t(s, j)      [ncols, ncols], the full symmetric matrix,
                         diagonal included, NOT divided by n_rows
   snpm_panel_loadings:  load[s][c] = sum over listed columns i of t(s, i) * vec[i][c]   vec [ncols, k], load [n_rows, k]
   The arithmetic is fp64 fused multiply-add throughout.  There are no floating-point atomics: every output cell has one owner and
   a summation order fixed by the arguments and the workspace budget, so two calls with the same arguments and settings return the
   same bits, and gram is symmetric bit for bit.  When every partial sum is exactly representable (tables of small integers) the
   result is the exact integer whatever the order; otherwise it differs from the exactly rounded sum by at most the bound of any
   summation order, n * 2^-53 * sum |t| |t| (n = n_rows) resp. sum |t| |vec| (n = ncols) to first order.
   snpm_panel_gram walks the row axis in slabs whose bit-planes (4 bits per call) and table rows fit a workspace budget (512 MiB;
   SNPM_PCA_WS_MB, read by snpm_init; a slab is at least one step of 1024 rows whatever the budget); the matrix accumulates on the
   device across slabs, in slab order.  Per slab a block owns a 64 x 64 tile pair for a run of plane steps (ceil(512 / tile pairs)
   runs, 1 .. 32), rows in order within the run, and the runs of a cell are added in order.  snpm_panel_loadings reads every selected
   row once from the panel itself, a wave per row: lane l sums columns l, l + 64, ... in order, six butterfly steps sum the lanes;
   its slabs (table rows and results inside the same budget, at least 64 rows) do not change the order.
   Limits: ncols <= SNPM_PCA_MAX_ACCESSIONS (kinship's: the matrix stays below 2^27 cells), 1 <= k <= SNPM_PCA_MAX_COMPONENTS,
   n_rows < 2^31.
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size, the
   limits, gram / vec non-NULL when ncols > 0, tab / load non-NULL when ncols > 0 and n_rows > 0, every entry of tab and vec finite
   (a NaN must never be multiplied by the 0 of a missing call) -- these before the panel handle is looked at, the message of a NULL
   panel is in snpm_last_error(NULL) -- then every column and row inside the panel, then ncols == the panel's accession count when
   cols is NULL.  ncols == 0 writes nothing and launches nothing; n_rows == 0 writes zeros to gram and nothing to load, without a
   launch.  Uploads into the panel that are still in flight are waited for on the device. */
#define SNPM_PCA_MAX_ACCESSIONS 11552
#define SNPM_PCA_MAX_COMPONENTS 32
int snpm_panel_gram(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                    const double *tab, double *gram);
int snpm_panel_loadings(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                        const double *tab, const double *vec, int k, double *load);

/* ---------------------------------------------------------------- admixture */
/* Joint EM iterations of the admixture model (STRUCTURE, FRAPPE, ADMIXTURE) on the accession columns of the RESIDENT panel (int8 or
   packed): every listed column is a mixture of K ancestral populations, every population has its own alt frequency at every
   selected row.  The package's own: the reference has no counterpart.  Host pointers in and out.
     cols, row_idx / row0 / n_rows   as for snpm_panel_gram (cols == NULL: all accessions; repeats count as listed)
     Q [ncols][K]    the ancestry of every listed column: entries >= 0, every row summing to 1
     F [n_rows][K]   the alt frequency of every component at every selected row, inside [SNPM_ADMIX_EPS, 1 - SNPM_ADMIX_EPS]
   The dosage g of a call from its canonical code: ref (0) g = 0, alt (1) g = 2, het (2) g = 1.  A missing call and an int8 panel's
   "other" code (3) are NO CALL: the cell contributes nothing anywhere.  One iteration maps (Q, F) to (Q', F'), BOTH read from the old
   pair (joint EM: the log-likelihood never decreases).  For a called cell (s, i):
     p = sum_k q_ik f_sk        pbar = sum_k q_ik (1 - f_sk)       both over k ascending with fma; pbar is its own positive sum,
                                                                   never 1 - p, so v and ln pbar stay accurate where p is close to 1
     u = g / p                  v = (2 - g) / pbar
     ll   = sum over cells of [g > 0] g ln p + [g < 2] (2 - g) ln pbar           (the likelihood of the OLD pair)
     a_sk = sum_i u q_ik        b_sk = sum_i v q_ik
     c_ik = sum_s (u f_sk + v (1 - f_sk))
     f'_sk = clamp(f a / (f a + (1 - f) b), EPS, 1 - EPS)       unchanged where the denominator is 0 (a row without a call)
     w_ik  = q_ik c_ik;  q'_ik = w_ik / sum_k w_ik (k ascending)  unchanged where that sum is 0 (a column without a call)
   With F inside [EPS, 1 - EPS] and the rows of Q summing to 1, p and pbar are at least EPS: no division by zero can occur.
     flags      SNPM_ADMIX_UPDATE_F | SNPM_ADMIX_UPDATE_Q: a component that is not updated keeps its bits (it is not written);
                flags == 0 only evaluates: loglik is written, Q and F come back untouched
     loglik [n_iter]   loglik[t] is the likelihood of the parameters at the START of iteration t
   Q and F are copied in once, stay on the device (double-buffered) for n_iter iterations and are copied out once.  All arithmetic
   is fp64 with IEEE division; there are no floating-point atomics: every output has one owner and one order of summation, a
   function of (n_rows, ncols, K) alone, so the same call returns the same bits, and n_iter = 3 returns the bits of three chained
   calls of one iteration.  a, b: lane l of a wave sums columns l, l + 64, ... in order, butterfly steps sum the lanes.  c: the rows
   go in contiguous runs (ceil(512 / ceil(ncols / 256)) of them, none below 16 rows), rows in order within a run, the runs are added
   in order.  ll: the same lanes, six butterfly steps, 32 rows in order per block, then a fixed tree of radix 4 over the blocks.
   Limits: 1 <= K <= SNPM_ADMIX_MAX_K, 1 <= n_iter <= 10000, ncols <= SNPM_PCA_MAX_ACCESSIONS, n_rows < 2^31.  There is no workspace
   knob and there are no row slabs: F and F' take 2 x n_rows x Kp x 8 bytes on the device (Kp = 4 / 8 / 16), the row list 8 bytes
   per row; what does not fit is reported (SNPM_ERR_OOM).
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size, the
   limits, no unknown flag bit, Q / loglik non-NULL when ncols > 0, F non-NULL when ncols > 0 and n_rows > 0, every entry of Q finite
   and >= 0, every row sum of Q within 1e-9 of 1, every entry of F finite and inside [EPS, 1 - EPS] -- these before the panel handle is
   looked at, the message of a NULL panel is in snpm_last_error(NULL) -- then every column and row inside the panel, then ncols ==
   the panel's accession count when cols is NULL.  ncols == 0 writes nothing and launches nothing; n_rows == 0 writes zeros to
   loglik, leaves Q and F, and launches nothing.  Uploads into the panel that are still in flight are waited for on the device. */
#define SNPM_ADMIX_MAX_K 16
#define SNPM_ADMIX_EPS 1e-6
#define SNPM_ADMIX_UPDATE_F 1u
#define SNPM_ADMIX_UPDATE_Q 2u
int snpm_panel_admix(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                     int K, int n_iter, unsigned flags, double *Q, double *F, double *loglik /* [n_iter] */);

/* ---------------------------------------------------------------- mixture */
/* The read-count-weighted 2 x 2 table of EVERY ordered pair of listed accession columns against one sample's allele depths (the
   FORMAT AD field of a VCF) over panel rows: what the likelihood of "a pool of accession a with a fraction alpha of accession b"
   needs, for a contaminated or pooled sample -- on the RESIDENT panel (int8 or packed), as one call.  The package's own: the
   reference has no such scan.  Host pointers in and out.
     cols [ncols]     accession columns, any order, repeats allowed; NULL = all accessions (ncols must then be the panel's count)
     row_idx [n_rows] panel rows, any order, repeats allowed; NULL = the dense range [row0, row0 + n_rows)
     alt, ref [n_rows]   the sample's reads of the alt and of the ref allele at every selected row, 0 .. 255 each
   On canonical DB codes (0, 1, 2, 3 = an int8 panel's "other" code, missing) a row counts for the pair (a, b) where BOTH columns
   carry a homozygous call (0 or 1); a het, "other" or missing call on either side drops the row for that pair.
     table [2][2][2][ncols][ncols]   table[w][ca][cb][a][b] = the sum, over the selected rows where column a has call ca and
                                     column b has call cb, of the sample's alt (w = 0) or ref (w = 1) reads
   Exact int32 sums; table[w][ca][cb][a][b] == table[w][cb][ca][b][a]; on the diagonal ca != cb gives 0 and ca == cb the sums of a
   column on its own.  The row axis is processed in slabs whose bit-planes (4 bits per call) fit a workspace budget (512 MiB;
   SNPM_MIX_WS_MB, read by snpm_init); two launches per slab, the sums accumulate on the device, so the result does not depend on
   the budget.  The counts travel as 2, 4 or 8 bit slices each: the smallest that hold the largest count of the call.
   Limits: ncols <= SNPM_MIX_MAX_ACCESSIONS (the tile pairs of the count kernel stay below 2^16), n_rows < 2^31, and
   n_rows * the largest byte of alt / ref < 2^31 (the sums are int32).
   Validated on the host before the device is touched (SNPM_ERR_BADARG with a message that names the rule): no negative size, the
   limits, non-NULL table when ncols > 0, non-NULL alt and ref when n_rows > 0, the int32 rule -- these before the panel handle is
   looked at, the message of a NULL panel is in snpm_last_error(NULL) -- then every column and row inside the panel, then ncols ==
   the panel's accession count when cols is NULL.  ncols == 0 writes nothing; n_rows == 0 writes zeros without a launch.  Uploads
   into the panel that are still in flight are waited for on the device. */
#define SNPM_MIX_MAX_ACCESSIONS 11552
int snpm_panel_mix_counts(snpm_panel *panel, const int32_t *cols, int64_t ncols, const int64_t *row_idx, int64_t row0, int64_t n_rows,
                          const uint8_t *alt, const uint8_t *ref, int32_t *table /* [2][2][2][ncols][ncols] */);

/* ---------------------------------------------------------------- sample input: VCF text (host only, no GPU) */
/* Single pass over a (plain or gzip) VCF: what ParseInputs.read_vcf (core/parsers.py:178-213, scikit-allel in
   the reference) extracts for sample column `sample_index`: CHROM, POS, the GT text as written, the first three
   PL values (-1 where absent) and INFO/DP (-1 where absent).  The calling thread reads (and inflates) the file in blocks of
   whole lines, a team of threads (the process's cores, at most 16; SNPM_VCF_THREADS) parses the blocks, file order is kept.
   SNPM_ERR_STATE = the file holds something this reader does not want to interpret (odd numbers, CRLF, very wide records):
   use the generic reader. */
typedef struct snpm_vcf snpm_vcf;
int snpm_vcf_parse(const char *path, int sample_index, snpm_vcf **out);
/* flags: bit 0 some FORMAT has GT, bit 1 some record has PL, bit 2 some record has INFO/DP, bit 3 CHROM / GT text is pure ASCII,
   bit 4 some FORMAT has DP (snpm_vcf_parse_calls_dp only) */
int snpm_vcf_dims(const snpm_vcf *vcf, int64_t *n_records, int *chr_width, int *gt_width, int *flags, int *n_samples);
/* chr [n * chr_width] and gt [n * gt_width]: NUL-padded fixed-width bytes; pos [n]; pl [n * 3]; dp [n] */
int snpm_vcf_fill(const snpm_vcf *vcf, char *chr, int64_t *pos, char *gt, double *pl, int64_t *dp);
/* The same with CHROM / GT as fixed-width UTF-32 (numpy '<U{width}': one code point per uint32_t, zero padded: no per-string
   conversion on the Python side) and called [n] = 0 where the genotype is './.' or '.|.' (the records ParseInputs.read_vcf
   drops, core/parsers.py:141-157).  SNPM_ERR_STATE when the text is not ASCII (flag bit 3). */
int snpm_vcf_fill_u32(const snpm_vcf *vcf, uint32_t *chr, int64_t *pos, uint32_t *gt, double *pl, int64_t *dp, uint8_t *called);
const char *snpm_vcf_sample_name(const snpm_vcf *vcf, int i);
int snpm_vcf_free(snpm_vcf *vcf);
/* The same single pass for EVERY sample column (genotype_cross reads a multi-sample VCF of F2 individuals): per record CHROM, POS
   and one call code per sample -- bits 0-2 the class (0 '0s0', 1 '1s1', 2 '0s1' / '1s0', 3 '.s.', 4 any other text with a
   separator s), bit 3 set when s is '|', 0xFF for a genotype without a separator -- instead of the GT text.  Declines
   (SNPM_ERR_STATE) where snpm_vcf_parse does, and when a record does not carry exactly the header's sample columns.  Sizes through
   snpm_vcf_dims (n_records, chr_width, n_samples); snpm_vcf_fill_calls writes chr [n * chr_width] as UTF-32, pos [n] and
   codes [n, ld] (ld >= n_samples, the samples of a record contiguous; bytes past n_samples are left alone). */
int snpm_vcf_parse_calls(const char *path, snpm_vcf **out);
int snpm_vcf_fill_calls(const snpm_vcf *vcf, uint32_t *chr, int64_t *pos, uint8_t *codes, int64_t ld);
/* snpm_vcf_parse_calls that also keeps the FORMAT DP subfield of every sample column (genotype_cross_hmm): the same records,
   codes and refusals; snpm_vcf_dims reports flag bit 4 when some FORMAT carries DP.  snpm_vcf_fill_calls_dp writes dp [n, ld]
   (ld >= n_samples): the integer as written, -1 for '.', for an entry that ends before its DP subfield and for a FORMAT without
   DP (scikit-allel's fill value).  A DP text that is not a plain integer of at most 9 digits declines the file. */
int snpm_vcf_parse_calls_dp(const char *path, snpm_vcf **out);
int snpm_vcf_fill_calls_dp(const snpm_vcf *vcf, int32_t *dp, int64_t ld);

/* ---------------------------------------------------------------- DB input: the reference's HDF5 files (host only, no GPU) */
/* A reader for the files the reference keeps its DBs in -- `snps` int8 [num_snps, num_accessions] in lzf chunks of (1000,
   num_accessions), `positions` with the attributes `chrs` / `chr_regions`, `accessions` (pygwas/genotype.py:310-326), and the
   accession-major twin in gzip chunks (core/makedb.py:64-81) -- for hosts without h5py / libhdf5.  Scope: files of the default
   ("earliest") format of HDF5 1.8 / 1.10: superblock 0-3 with version-1 object headers, old-style groups, compact / contiguous /
   chunked (version-1 B-tree) layouts, filters gzip, shuffle, lzf, integer / float / fixed- and variable-length string data,
   little-endian.  Anything else returns SNPM_ERR_BADARG with a message in snpm_h5_last_error(file) (file == NULL: of the last
   failed snpm_h5_open in this thread).  snpm_h5 handles are independent of contexts; reads are thread-safe. */
typedef struct snpm_h5 snpm_h5;
int snpm_h5_open(const char *path, snpm_h5 **out);
int snpm_h5_close(snpm_h5 *file);
const char *snpm_h5_last_error(const snpm_h5 *file);
/* member names of a group ("" = root), '\n'-separated; *needed = bytes incl. the terminating NUL */
int snpm_h5_list(snpm_h5 *file, const char *group, char *buf, int64_t cap, int64_t *needed);
/* object `path` (attr == NULL) or its attribute `attr`: kind 0 group / 1 data; rank, dims [8], type_class 0 integer / 1 float /
   3 string (variable-length strings are presented as fixed-length ones of elem_size = the longest), elem_size bytes, chunk [8]
   (0s: not chunked), number of attributes.  Any output may be NULL. */
int snpm_h5_info(snpm_h5 *file, const char *path, const char *attr, int *kind, int *rank, int64_t *dims, int *type_class,
                 int *elem_size, int *is_signed, int64_t *chunk, int *n_attrs);
int snpm_h5_attr_name(snpm_h5 *file, const char *path, int index, char *buf, int64_t cap);
/* the whole dataset / attribute in C order; out_bytes = elements * elem_size as snpm_h5_info reports them */
int snpm_h5_read(snpm_h5 *file, const char *path, const char *attr, void *out, int64_t out_bytes);
/* rows row_idx[i] (or file_row0 + i when row_idx is NULL), columns [col0, col0 + ncols) of a 1-D / 2-D dataset of fixed-size
   elements (the reference's g.g.snps[idx, :] / g.g_acc.snps[:, i]) -> out, row stride out_pitch BYTES */
int snpm_h5_read_rows(snpm_h5 *file, const char *path, const int64_t *row_idx, int64_t file_row0, int64_t nrows, int64_t col0,
                      int64_t ncols, void *out, int64_t out_pitch);
/* snpm_panel_load_file_rows for a 2-D int8 dataset of an open HDF5 file: chunks are read and decompressed by the loader's host
   threads straight into the pinned staging slabs (packed panels: packed there too) */
int snpm_panel_load_h5(snpm_panel *panel, snpm_h5 *file, const char *dataset, int64_t col0, const int64_t *row_idx,
                       int64_t file_row0, int64_t row0, int64_t nrows);

#ifdef __cplusplus
}
#endif
#endif /* SNPMATCH_HIP_H */
