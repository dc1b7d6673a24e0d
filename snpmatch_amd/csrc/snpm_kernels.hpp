// snpm_kernels.hpp -- hand-written HIP kernels for gfx950 (MI355X, wave64) behind libsnpmatch_hip.so.
//
// The work is compare-and-count over an int8 SNP x accession panel: HBM-bound byte streaming,
// no MFMA.  Layout: panel is SNP-major [n_snp, pitch] (pitch = n_acc rounded up to 256 B), so one
// SNP row is a coalesced run of accession bytes and the three weights of a row are wave-uniform.
//
// Kernels
//   k_fast     dominant kernel.  Each lane owns BPL adjacent accessions (one 4/8/16-byte load per
//              row), each wave 64*BPL adjacent accession bytes, each workgroup a run of rows (a "part").
//              Per-row weights live in LDS as a 4-entry fp64 LUT {ref, alt, het, 0} indexed by
//              (byte & 3); every element costs one ds_read_b64 + one v_add_f64 instead of three
//              compare/select pairs.  Missing counts are SWAR (packed u8 lanes).  Partials per part
//              are written once; k_reduce adds them in part order (deterministic, no atomics).
//   k_fast_packed_q4 the fast pass on a 2-bit packed panel: 16 accessions per lane, four rows per table lookup
//              (one ds_read_b128 + two v_add_f64 per two comparisons), bit-sliced missing counts, LDS reads
//              issued and waited for by hand.
//   k_fast_bits  hard-call samples (all weights 0 or 1) on a packed panel: bit-plane boolean scoring and
//              bit-sliced counting, no LDS, no fp64.
//   k_strict4 / k_strict_sparse(_T)  reference summation order (three per-category sequential fp64
//              sums per segment, core/snpmatch.py:85-87).  Used for cross windows, for SNPM_MODE_STRICT and to
//              re-evaluate the few accessions the fast pass cannot certify (sparse variants; _T reads the
//              accession-major packed copy built by k_pack_transpose).
//   k_scan / k_scan_few  sequential accumulation of segment sums (ScoreList += chunk, core/snpmatch.py:224), with an
//              optional carry-in (totals of earlier SNP slabs).
//   k_fast<..., SEG>  the same fast pass over many independent row ranges (samples of a batch, windows of a cross) in one
//              launch; k_reduce_seg / k_eseg_part + k_eseg_finish / k_strict_pairs / k_scan_pairs: per-segment reduce, error bound, and the
//              reference-order re-evaluation of the (segment, accession) pairs the certificate flags.
//   certificate  k_wprops (weight properties), k_eref / k_efinish (reference-order error bound on the device),
//              k_chunk_sums / k_echain (the same bound for one slab of a slab-streamed job, chain additions charged by the
//              magnitude of the running total), flag_if_uncertain inside k_reduce / k_carry_flag; the re-evaluation kernels read the flag count on the
//              device and leave at once when their tier has nothing to do (dense_tier_off, *d_ncols).
//   k_carry_add / k_carry_flag / k_tot_seg  running totals of slab-streamed jobs, totals over windows.
//   k_likelihood  likeliTest + nanmin + ratio on device (core/snpmatch.py:40-55,106-117).
//   k_binom_identity  np_test_identity (core/snpmatch.py:57-72).   k_segregating  --refine support.
//   k_gcross   genotype_cross: m1 / mh / m2 counts per (window, F2 sample) and the three-way likelihood decision (core/genotype_cross.py:21-49).
//   k_ghmm     genotype_cross_hmm: the 3-state Viterbi path of every (chromosome, F2 sample), one chain per lane, tables of logarithms from the host (core/infer.py:17-58).
//   k_pair_transpose / k_pair_count  pairsnp: genotype-text ids of a cohort, sample-major planes, byte-parallel compare-and-count of every pair of samples per chromosome (core/snpmatch.py:270-309).
//   k_kin_planes / k_kin_count  panel kinship: accession-major bit-planes (ref / alt / informative) of a slab of panel rows, AND + popcount of every pair of accessions, 64 rows per word (core/snp_genotype.py:256-289, :440-459).
//   k_site_counts  site statistics: c0 / c1 / c2 / ninfo of every selected panel row per group of accession columns, AND + popcount of indicator words against membership words held in LDS, a row per part of a wave (core/snp_genotype.py:119-175, :360-376, :385-394).
//   k_ld_planes / k_ld_band  panel LD: member-masked bit-planes (alt / het / informative) of a slab of panel rows and its halo, the nine AND + popcount counts and r2 of every row with each of the `band` rows after it, a pair per lane (core/snp_genotype.py:291-295, :348-358).
//   k_win_planes / k_win_count  panel windows: accession-major bit-planes (ref / alt / het / informative) of a slab of panel rows, masked popcounts per genome window of every column and of listed pairs of columns, a group of lanes per cell (core/snp_genotype.py:297-345).
//   k_f1x_count  f1search: the in-silico F1 of EVERY pair of accession columns against one sample's hard calls -- the four planes of k_win_planes, a fifth made while staging, three sample masks; hits / ninfo by AND / XOR + popcount, 64 rows per word (the exhaustive form of core/csmatch.py:106-129).
//   k_par_count  parentsearch: every pair of accession columns per genome window as parent A, parent B or their F1, whichever fits the sample best there -- the planes and tiling of k_f1x_count, window boundaries folded into a stream of masked segments, a maximum per whole window.
//   k_sim_noise / k_sim_count  power: call errors injected into the planes of k_win_planes by a counter-based hash (the sample simulated from every accession column), then score / ninfo of every ORDERED pair (sample of a, DB column b) per group of selected rows -- the tiling of k_f1x_count over the full square of tile pairs, group boundaries as bit masks (the all-accessions form of core/simulate.py:26-53 + core/snpmatch.py:74-117).
//   k_mos_fwd / k_mos_back  mosaic: the copying-model Viterbi (uniform switch cost, integer costs) of every (chain, sample) with the accession columns as states -- the planes of k_win_planes folded with the sample's class words into cost bit-planes once per 64 rows, V of a thread's columns in registers, one (minimum, lowest column) per row by ballots (one where the copied column matched), a 32-bit key per wave and one barrier; the path walked back by one wave per chain, a load per word without a switch.
//   k_ibd_count / k_ibd_runs  ibd: for every pair of accession columns the genome windows in which the two are identical -- planes P0 and P1 of k_win_planes, the tiling and the segment stream of k_par_count with two planes per side, n / d by AND / XOR + popcount, two integer rules per whole window into totals and two window bitsets; then a thread per cell walks the bitsets into runs.
//   k_mk_rowplanes / k_mk_gain / k_mk_pick / k_mk_update  markers: a greedy minimal set of panel rows that separates every pair of accession columns -- bit-planes the other way round (one bit per accession, one word row per SNP, a ballot per word), per round the gain of every eligible row by AND + popcount against the bit matrix of unresolved pairs, the best row from one key per gain block, the need matrix decremented cell by cell and the bit matrix rebuilt by ballot.
//   k_pca_gram / k_pca_fold / k_pca_load  pca: the class-table-weighted Gram matrix of the accession columns -- the planes of k_win_planes decoded to fp64 values in LDS, a 64 x 64 tile pair and a run of plane steps per block, a 4 x 4 register tile of fp64 FMAs per lane, partial sums with one owner each folded into the matrix in a fixed order -- and the loadings, a wave per panel row (the package's own: no counterpart in the reference).
//   k_adm_rows / k_adm_cols / k_adm_fold  admixture: one joint EM iteration of the model of STRUCTURE / ADMIXTURE -- a wave per panel row for the new frequencies and the likelihood, a thread per accession column and run of rows for the new ancestries, partial sums with one owner each folded in a fixed order, the likelihood in a fixed tree; all fp64, IEEE division (the package's own: no counterpart in the reference).
//   k_mix_count<2 / 4 / 8>  mixture: the read-count-weighted 2 x 2 table of EVERY ordered pair of accession columns against one sample's allele depths (FORMAT AD) -- planes P0 and P1 of k_win_planes, the tiling of k_f1x_count, the alt and ref counts as 2 / 4 / 8 bit slices each; eight int32 sums per pair by AND + popcount + shift, 64 rows per word (the package's own: no counterpart in the reference).
//   k_f1_*     in-silico F1 scores in numpy's summation order (core/csmatch.py:115-125).
//   k_build_lut, k_repitch_canon / k_pack_rows / k_unpack_rows (upload / download), k_pack_transpose[_packed]
//   (accession-major copies), k_synth* / k_synth_sample (benchmark data), k_check_rows, k_expand_codes, k_seg_pack,
//   k_patch, k_calib_read: small helpers.
//
// The kernels live in one header per family; this file only puts them together (order matters: later families use the
// constants and helpers of earlier ones):
#pragma once
#include "snpm_k_common.hpp"      // build switches, constants
#include "snpm_k_prep.hpp"        // k_build_lut, k_wprops, k_wbits, k_eref / k_efinish, k_chunk_sums / k_echain, k_check_rows, k_expand_codes
#include "snpm_k_fast.hpp"        // k_fast
#include "snpm_k_packed.hpp"      // k_fast_packed_q4, k_fast_bits
#include "snpm_k_reduce.hpp"      // k_reduce*, k_carry_*, k_eseg_*, k_reduce_seg, k_strict_pairs, k_scan_pairs, k_tot_seg, helpers
#include "snpm_k_strict.hpp"      // k_strict4, k_strict_sparse(_T), k_pack_transpose*, k_scan, k_scan_few, k_seg_pack, k_patch
#include "snpm_k_shared.hpp"      // k_sh_*: the shared-row scan of a batch (int8 MFMA contraction of fixed-point weight digits with the one-hot panel)
#include "snpm_k_post.hpp"        // k_likelihood, k_binom_identity, k_segregating, k_f1_*, k_once_pack
#include "snpm_k_gcross.hpp"      // k_gcross (genotype_cross: per window and sample parental calls)
#include "snpm_k_ghmm.hpp"        // k_ghmm (genotype_cross_hmm: one Viterbi chain per lane)
#include "snpm_k_pairs.hpp"       // k_pair_transpose, k_pair_count (pairsnp: common / matching records of every pair of samples)
#include "snpm_k_kin.hpp"         // k_kin_planes, k_kin_count (panel kinship: ninfo / same / diff of every pair of accessions)
#include "snpm_k_site.hpp"        // k_site_counts (site statistics: per-row allele counts per group of accessions)
#include "snpm_k_ld.hpp"          // k_ld_planes, k_ld_band (panel LD: nine counts and r2 of every row pair within a band)
#include "snpm_k_win.hpp"         // k_win_planes, k_win_count (panel windows: per-window counts of every column and of listed column pairs)
#include "snpm_k_f1x.hpp"         // k_f1x_count (f1search: hits / ninfo of the in-silico F1 of every pair of accessions against a sample)
#include "snpm_k_par.hpp"         // k_par_count (parentsearch: every pair of accessions per genome window as the parents of a recombinant sample)
#include "snpm_k_sim.hpp"         // k_sim_noise, k_sim_count (power: the sample simulated from every accession scored against every accession, per group of rows)
#include "snpm_k_mos.hpp"         // k_mos_fwd, k_mos_back (mosaic: the copying-model Viterbi path of every chain and sample over the accession columns)
#include "snpm_k_ibd.hpp"         // k_ibd_count, k_ibd_runs (ibd: the windows in which every pair of accessions is identical, and the runs they form)
#include "snpm_k_mk.hpp"          // k_mk_rowplanes, k_mk_gain, k_mk_pick, k_mk_update (markers: a greedy minimal set of rows that separates every pair of accessions)
#include "snpm_k_pca.hpp"         // k_pca_gram, k_pca_fold, k_pca_load (pca: the weighted Gram matrix of the accession columns and the row-streaming product for the loadings)
#include "snpm_k_adm.hpp"         // k_adm_rows, k_adm_cols, k_adm_fold (admixture: one joint EM iteration of the ancestry model over the accession columns)
#include "snpm_k_mix.hpp"         // k_mix_count (mixture: alt / ref read sums per pair of homozygous calls of every ordered pair of accessions)
#include "snpm_k_io.hpp"          // k_pack_rows, k_repitch_canon, k_unpack_rows, k_synth*, k_calib_read
#include "snpm_kernels_single.hpp"   // k_strict_single (panels of one accession: numpy's pairwise order)
