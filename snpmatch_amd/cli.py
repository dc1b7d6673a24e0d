"""
Command line, one subcommand (or group of them) per line:

  * ``snpmatch inbred``, ``snpmatch cross`` and ``snpmatch genotype_cross`` with the reference's flags (snpmatch/__init__.py:44-78), logging setup (:23-34) and exit codes (:155-183), plus ``makedb-native`` to write the flat panel format this engine streams to the GPU.
  * ``genotype_cross`` serves the windowed likelihood-ratio mode with the parents named as two accessions of the database (``-p 6091x6191``); the HMM genotyper of the reference's ``--hmm`` flag is the subcommand ``genotype_cross_hmm``.  ``--hmm`` itself and ``-q / --father`` are refused with a message (core/genotype_cross.py says why).
  * ``pairsnp`` compares two sample files as the reference does; ``pairsnp-batch`` compares every pair of a cohort in one device call.
  * ``kinship`` (not in the reference as a command) counts the relatedness of every pair of accessions of the database on the device and lists the near-identical ones.
  * ``sitestats`` (not in the reference as a command either) counts the alleles of every DB row per population on the device and writes frequencies, missingness and a site filter.
  * ``ld`` (the reference's ``calculate_ld`` does not run) computes r2 of neighbouring DB rows inside a band on the device and prunes the rows by it.
  * ``windows`` (not in the reference as a command) counts, per genome window, the heterozygosity of every accession and the mismatch of listed pairs of accessions on the device.
  * ``f1search`` (not in the reference) scores the in-silico F1 of EVERY pair of accessions against a sample on the device, where ``cross`` tries the ten best singles.
  * ``mixture`` (not in the reference) reads the allele depths (FORMAT AD) of a sample and fits "accession a with a fraction alpha of accession b" to EVERY ordered pair of accessions from read sums counted on the device: a contaminated or pooled sample, which ``inbred`` and ``f1search`` do not see.
  * ``parentsearch`` (not in the reference) scores every pair of accessions per genome window as the parents of a recombinant sample (an F2, a backcross), where the sample is parent A in one window, the F1 in the next and parent B in a third.
  * ``simulate`` draws a test sample from the database as the reference does (host only, the same draws under one ``--seed``).
  * ``power`` (not in the reference) simulates a sample from EVERY accession and scores it against every accession on the device, for a whole ladder of marker counts: which accessions ``inbred`` identifies uniquely with n SNPs at a call error rate, and whom it confuses.
  * ``mosaic`` (not in the reference) paints a sample of more than two sources -- a MAGIC line, a multi-parent RIL, an admixed sample -- as a mosaic of the accessions of the database on the device: the copying-model Viterbi path with a uniform switch cost, every accession a state.
  * ``ibd`` (not in the reference) finds, for EVERY pair of accessions of the database, the genome windows in which the two are identical and the runs of such windows along each chromosome: shared haplotype segments.
  * ``markers`` (not in the reference) chooses a small set of SNPs that separates EVERY pair of accessions of the database on the device -- the greedy set cover, round by round inside one device call: the SNPs to genotype so that no two accessions are confused.
  * ``pca`` (not in the reference) makes the genotype relationship matrix of the accessions on the device (an fp64 rank-R update, every row weighted by its allele frequency), decomposes it and projects samples onto its principal axes: which part of the collection a sample that matches no accession belongs to.
  * ``admixture`` (not in the reference) fits the admixture model of STRUCTURE / ADMIXTURE -- every accession a mixture of K ancestral populations -- by joint EM on the device, the parameters resident between iterations, and writes the population file the other panel commands take as ``--pops``.

The other reference subcommands (parser, makedb) are outside the accelerated path.
"""
import argparse
import logging
import os
import sys

__version__ = "0.1.0 (SNPmatch 5.0.1 inbred/cross interface)"


def setLog(logDebug):
    log = logging.getLogger()
    numeric_level = logging.DEBUG if logDebug else logging.ERROR
    log_format = logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s")
    lch = logging.StreamHandler()
    lch.setLevel(numeric_level)
    lch.setFormatter(log_format)
    log.setLevel(numeric_level)
    log.addHandler(lch)


def die(msg):
    sys.stderr.write('Error: ' + msg + '\n')
    sys.exit(1)


def check_file(inFile):
    if not inFile:
        die("file: %s not specified" % inFile)
    if not os.path.exists(inFile):
        die("input file does not exist: " + inFile)


def check_files(args, required=(), optional=()):
    """``check_file`` on the files a subcommand needs and on those of its optional files that are given"""
    for key in required:
        check_file(args[key])
    for key in optional:
        if args.get(key):
            check_file(args[key])


def snpmatch_inbred(args):
    from .core import snpmatch
    check_file(args['inFile'])
    snpmatch.potatoGenotyper(args)


def snpmatch_inbred_batch(args):
    from .core import snpmatch
    for f in args['inFiles']:
        check_file(f)
    snpmatch.potatoGenotyperBatch(args)


def snpmatch_cross(args):
    from .core import csmatch
    check_file(args['inFile'])
    csmatch.potatoCrossIdentifier(args)


def snpmatch_genotype_cross(args):
    from .core import genotype_cross
    if args['hmm']:
        die(genotype_cross.HMM_REFUSED)
    if args['father'] is not None:
        die(genotype_cross.FATHER_REFUSED)
    check_file(args['inFile'])
    if not args['parents']:
        die("parents not specified: -p 6091x6191")
    genotype_cross.potatoCrossGenotyper(args)


def snpmatch_genotype_cross_hmm(args):
    from .core import genotype_cross
    check_file(args['inFile'])
    if not args['parents']:
        die("parents not specified: -p 6091x6191")
    genotype_cross.potatoCrossGenotyper(dict(args, hmm=True, father=None, binLen=0, lr_thres=None))


def snpmatch_paircomparions(args):
    from .core import snpmatch
    check_file(args['inFile_1'])
    check_file(args['inFile_2'])
    snpmatch.pairwiseScore(args['inFile_1'], args['inFile_2'], args['logDebug'], args['outFile'], args['hdf5File'])


def snpmatch_pair_cohort(args):
    from .core import pairsnp
    for f in args['inFiles']:
        check_file(f)
    pairsnp.potatoPairCohort(args)


def snpmatch_kinship(args):
    from .core import kinship
    check_files(args, ('hdf5File',), ('accFile',))
    kinship.potatoKinship(args)


def snpmatch_sitestats(args):
    from .core import sitestats
    check_files(args, ('hdf5File',), ('accFile', 'popFile'))
    sitestats.potatoSiteStats(args)


def snpmatch_ld(args):
    from .core import ld
    check_files(args, ('hdf5File',), ('accFile', 'sitesFile'))
    ld.potatoLD(args)


def snpmatch_windows(args):
    from .core import windows
    check_files(args, ('hdf5File',), ('accFile', 'pairsFile'))
    windows.potatoWindows(args)


def snpmatch_f1search(args):
    from .core import f1search
    check_files(args, ('inFile', 'hdf5File'), ('accFile',))
    f1search.potatoF1Search(args)


def snpmatch_mixture(args):
    from .core import mixture
    check_files(args, ('inFile', 'hdf5File'), ('accFile', 'sitesFile'))
    mixture.potatoMixture(args)


def snpmatch_parentsearch(args):
    from .core import parentsearch
    check_files(args, ('inFile', 'hdf5File'), ('accFile',))
    parentsearch.potatoParentSearch(args)


def snpmatch_simulate(args):
    from .core import simulate
    check_file(args['hdf5File'])
    if not args['AccID']:
        die("accession not specified: -a 6091 (or -a 6091x6191 with --f1)")
    if args['numSNPs'] is None or args['numSNPs'] < 0:
        die("number of SNPs not specified: -n 1000")
    simulate.potatoSimulate(args)


def snpmatch_power(args):
    from .core import power
    check_files(args, ('hdf5File',), ('accFile', 'sitesFile'))
    power.potatoPower(args)


def snpmatch_mosaic(args):
    from .core import mosaic
    check_files(args, ('inFile', 'hdf5File'), ('accFile',))
    mosaic.potatoMosaic(args)


def snpmatch_ibd(args):
    from .core import ibd
    check_files(args, ('hdf5File',), ('accFile',))
    ibd.potatoIBD(args)


def snpmatch_markers(args):
    from .core import markers
    check_files(args, ('hdf5File',), ('accFile', 'sitesFile'))
    markers.potatoMarkers(args)


def snpmatch_admixture(args):
    from .core import admixture
    check_files(args, ('hdf5File',), ('accFile', 'popFile', 'sitesFile', 'inFile'))
    admixture.potatoAdmixture(args)


def snpmatch_pca(args):
    from .core import pca
    check_files(args, ('hdf5File',), ('accFile', 'popFile', 'sitesFile', 'inFile'))
    pca.potatoPCA(args)


def makedb_native(args):
    """<db>.npz (snps, accessions, positions, chrs, chr_regions) or HDF5 -> <out>.snpm flat panel"""
    from .core import snp_genotype
    g = snp_genotype._load_any(args['inFile'])
    snp_genotype.save_native(args['outFile'], g.snps, g.accessions, g.positions, g.chrs, g.chr_regions, packed=args.get('packed', False))


def get_options(description, version_message):
    p = argparse.ArgumentParser(description=description)
    p.add_argument('-V', '--version', action='version', version=version_message)
    sub = p.add_subparsers(title='subcommands', description='Choose a command to run', help='Following commands are supported')

    def db_options(sp, required=True):
        sp.add_argument("-d", "--hdf5_file", default=None, dest="hdf5File", required=required, help="Path to SNP matrix (as for inbred)")
        sp.add_argument("-e", "--hdf5_acc_file", default=None, dest="hdf5accFile", help="Path to SNP matrix chunked column-wise (optional for flat panels)")

    def verbose(sp):
        sp.add_argument("-v", "--verbose", action="store_true", dest="logDebug", default=False, help="Show verbose debugging output")

    def common(sp, default_out):
        sp.add_argument("-i", "--input_file", dest="inFile", help="VCF/BED file for the variants in the sample")
        sp.add_argument("-d", "--hdf5_file", default=None, dest="hdf5File",
                        help="Path to SNP matrix: native flat panel directory (.snpm), .npz, or HDF5 chunked row-wise")
        sp.add_argument("-e", "--hdf5_acc_file", default=None, dest="hdf5accFile",
                        help="Path to SNP matrix chunked column-wise (optional for flat panels)")
        sp.add_argument("--skip_db_hets", action="store_true", dest="skip_db_hets", default=False,
                        help="Replace heterozygous calls in DB with nan during the analysis.")
        verbose(sp)
        sp.add_argument("-o", "--output", dest="outFile", default=default_out, help="Output file prefix")

    inbred = sub.add_parser('inbred', help="SNPmatch on the inbred samples")
    common(inbred, "identify_inbred")
    inbred.add_argument("--refine", action="store_true", dest="refine", default=False, help="Refine scores for indistinguishable lines")
    inbred.set_defaults(func=snpmatch_inbred)

    # not in the reference (which starts a process, and opens the DB, per sample): many samples against ONE resident DB
    batch = sub.add_parser('inbred-batch', help="`inbred` for many samples: the DB is loaded once, samples are scored a batch per device call")
    batch.add_argument("-i", "--input_files", dest="inFiles", nargs='+', required=True, help="VCF/BED files, one sample each")
    db_options(batch, required=False)
    batch.add_argument("--skip_db_hets", action="store_true", dest="skip_db_hets", default=False,
                       help="Replace heterozygous calls in DB with nan during the analysis.")
    verbose(batch)
    batch.add_argument("-o", "--output", dest="outFile", default="identify_inbred",
                       help="Output prefix: sample <name>.vcf writes <prefix>.<name>.scores.txt / .matches.json")
    batch.add_argument("--batch_size", dest="batchSize", default=64, type=int, help="samples per device call")
    batch.set_defaults(func=snpmatch_inbred_batch)

    cross = sub.add_parser('cross', help="SNPmatch on the crosses (F2s and F3s) of A. thaliana")
    common(cross, "identify_cross")
    cross.add_argument("-b", "--binLength", dest="binLen", help="Length of bins to calculate the likelihoods", default=300000, type=int)
    cross.add_argument("--genome", dest="genome", default="athaliana_tair10",
                       help="Genome id or path to a reference JSON file (ref_chrs, ref_chrlen)")
    cross.set_defaults(func=snpmatch_cross)

    gcross = sub.add_parser('genotype_cross', help="Genotype F2 individuals of a cross: parent 1 / heterozygous / parent 2 per genome window")
    gcross.add_argument("-i", "--input_file", dest="inFile", help="multi-sample VCF file of the F2 individuals")
    gcross.add_argument("-d", "--hdf5_file", default=None, dest="hdf5File",
                        help="Path to SNP matrix: native flat panel directory (.snpm), .npz, or HDF5 chunked row-wise")
    gcross.add_argument("-e", "--hdf5_acc_file", default=None, dest="hdf5accFile",
                        help="Path to SNP matrix chunked column-wise (optional for flat panels)")
    gcross.add_argument("-p", "--parents", dest="parents", help="Parents of the cross as two accessions of the database: 6091x6191")
    gcross.add_argument("-q", "--father", dest="father", default=None,
                        help="(refused) the reference's two-VCF form of naming the parents")
    gcross.add_argument("-b", "--binLength", dest="binLen", help="bin length", default=200000, type=int)
    gcross.add_argument("--genome", dest="genome", default="athaliana_tair10",
                        help="Genome id or path to a reference JSON file (ref_chrs, ref_chrlen, optionally recomb_rates)")
    gcross.add_argument("--lr_thres", dest="lr_thres", default=1.5, type=float,
                        help="likelihood ratio a parental call must reach over the next best class")
    gcross.add_argument("--good_samples", dest="good_samples", default=None, help="accepted and unused, as in the reference's own call path")
    gcross.add_argument("--hmm", action="store_true", dest="hmm", default=False, help="(refused) the reference's HMM genotyper")
    gcross.add_argument("-o", "--output", dest="outFile", default="genotype_cross", help="output file")
    verbose(gcross)
    gcross.set_defaults(func=snpmatch_genotype_cross)

    ghmm = sub.add_parser('genotype_cross_hmm', help="Genotype F2 individuals of a cross marker by marker (AA / AB / BB) with a 3-state HMM")
    ghmm.add_argument("-i", "--input_file", dest="inFile", help="multi-sample VCF file of the F2 individuals, DP in its FORMAT")
    ghmm.add_argument("-d", "--hdf5_file", default=None, dest="hdf5File",
                      help="Path to SNP matrix: native flat panel directory (.snpm), .npz, or HDF5 chunked row-wise")
    ghmm.add_argument("-e", "--hdf5_acc_file", default=None, dest="hdf5accFile",
                      help="Path to SNP matrix chunked column-wise (optional for flat panels)")
    ghmm.add_argument("-p", "--parents", dest="parents", help="Parents of the cross as two accessions of the database: 6091x6191")
    ghmm.add_argument("--genome", dest="genome", default="athaliana_tair10",
                      help="Genome id or path to a reference JSON file (ref_chrs, ref_chrlen, optionally recomb_rates)")
    ghmm.add_argument("-o", "--output", dest="outFile", default="genotype_cross_hmm", help="output file")
    verbose(ghmm)
    ghmm.set_defaults(func=snpmatch_genotype_cross_hmm)

    pair = sub.add_parser('pairsnp', help="pairwise comparison of two snp files")
    pair.add_argument("-i", "--input_file_1", dest="inFile_1", help="VCF/BED file for the variants in the sample one")
    pair.add_argument("-j", "--input_file_2", dest="inFile_2", help="VCF/BED file for the variants in the sample two")
    pair.add_argument("-d", "--hdf5_file", dest="hdf5File", default=None,
                      help="Path to SNP matrix (as for inbred): only positions the database holds are compared")
    verbose(pair)
    pair.add_argument("-o", "--output", dest="outFile", default="pairsnp", help="output json file")
    pair.set_defaults(func=snpmatch_paircomparions)

    # not in the reference (one process per pair of files): every pair of a plate or sequencing batch in ONE device call
    pairs = sub.add_parser('pairsnp-batch', help="`pairsnp` for every pair of a cohort: one multi-sample VCF, or several files of one sample each")
    pairs.add_argument("-i", "--input_files", dest="inFiles", nargs='+', required=True,
                       help="one multi-sample VCF, or VCF/BED files of one sample each")
    pairs.add_argument("-d", "--hdf5_file", dest="hdf5File", default=None,
                       help="Path to SNP matrix (as for inbred): only positions the database holds are compared")
    verbose(pairs)
    pairs.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.pairs.tsv and <prefix>.pairs.npz")
    pairs.set_defaults(func=snpmatch_pair_cohort)

    # not in the reference as a command (its Genotype.kinship_given_snps is a method): relatedness of every pair of accessions of the DB
    kin = sub.add_parser('kinship', help="kinship of every pair of accessions of the database, and the list of near-identical pairs")
    db_options(kin)
    kin.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    kin.add_argument("--bed", dest="bed", default=None, help="only the DB rows of a region: Chr1,1,1000000 (default: all rows)")
    kin.add_argument("--min_identity", dest="min_identity", default=0.99, type=float,
                     help="list a pair as duplicates from this share of equal calls among the rows where both are homozygous (default 0.99)")
    kin.add_argument("--min_sites", dest="min_sites", default=100, type=int,
                     help="... and only when both are homozygous at this many rows or more (default 100)")
    verbose(kin)
    kin.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.kinship.npz and <prefix>.duplicates.tsv")
    kin.set_defaults(func=snpmatch_kinship)

    # not in the reference as a command (its Genotype.get_af_snps is a method): allele counts and frequencies of every DB row per population
    site = sub.add_parser('sitestats', help="allele counts, frequencies and missingness of every SNP of the database, per population")
    db_options(site)
    site.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line: one population of these (default: all accessions)")
    site.add_argument("--pops", dest="popFile", default=None, help="text file of two columns, accession and population (# lines are skipped): statistics per population")
    site.add_argument("--bed", dest="bed", default=None, help="only the DB rows of a region: Chr1,1,1000000 (default: all rows)")
    site.add_argument("--min_informative", dest="min_informative", default=0, type=int,
                      help="frequencies are nan where no more than this many accessions of the population carry a call (default 0)")
    site.add_argument("--min_maf", dest="min_maf", default=None, type=float, help="write <prefix>.sites.tsv: rows whose maf is at least this in every population")
    site.add_argument("--max_missing", dest="max_missing", default=None, type=float,
                      help="write <prefix>.sites.tsv: rows whose share of accessions without a call is at most this in every population")
    verbose(site)
    site.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.sitestats.npz, <prefix>.sitestats.json and, with a threshold, <prefix>.sites.tsv")
    site.set_defaults(func=snpmatch_sitestats)

    # not in the reference as a command (its calculate_ld does not run): LD between neighbouring SNPs of the DB and pruning of a marker set by it
    ldp = sub.add_parser('ld', help="linkage disequilibrium (r2) of every SNP with the SNPs after it inside a band, the decay curve, and LD pruning of the rows")
    db_options(ldp)
    ldp.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    ldp.add_argument("--bed", dest="bed", default=None, help="only the DB rows of a region: Chr1,1,1000000 (default: all rows)")
    ldp.add_argument("--sites", dest="sitesFile", default=None, help="only the rows listed in a <prefix>.sites.tsv of sitestats (columns chr and pos)")
    ldp.add_argument("--band", dest="band", default=50, type=int, help="pair every row with this many rows after it on its chromosome (default 50)")
    ldp.add_argument("--window_bp", dest="window_bp", default=None, type=int, help="pairs further apart than this many bp count as undefined")
    ldp.add_argument("--r2", dest="r2", default=0.2, type=float, help="prune a row whose r2 with an earlier kept row of the band exceeds this (default 0.2)")
    ldp.add_argument("--min_n", dest="min_n", default=2, type=int, help="r2 is undefined with fewer accessions informative at both rows (default 2)")
    ldp.add_argument("--keep_r2", action="store_true", dest="keep_r2", default=False, help="also write <prefix>.ld.npz: chr, pos, r2 [rows, band], keep")
    verbose(ldp)
    ldp.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.pruned.tsv and <prefix>.ld.json")
    ldp.set_defaults(func=snpmatch_ld)

    # not in the reference as a command (it has the two methods): per genome window, heterozygosity of the accessions and mismatch of pairs
    win = sub.add_parser('windows', help="per genome window: heterozygosity of every accession of the DB and mismatch of listed pairs of accessions (e.g. the duplicates of kinship)")
    db_options(win)
    win.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    win.add_argument("--pairs", dest="pairsFile", default=None, help="text file whose first two columns name pairs of the selected accessions (a <prefix>.duplicates.tsv of kinship goes straight in)")
    win.add_argument("--pairs_only", action="store_true", dest="pairs_only", default=False, help="take the members of the pairs as the accessions")
    win.add_argument("--genome", dest="genome", default="athaliana_tair10", help="Genome id or path to a reference JSON file (ref_chrs, ref_chrlen)")
    win.add_argument("-b", "--window_size", dest="binLen", default=300000, type=int, help="window length in bp (default 300000)")
    win.add_argument("--min_sites", dest="min_sites", default=5, type=int, help="a window is judged with MORE than this many informative rows; het is nan otherwise (default 5, the reference's)")
    verbose(win)
    win.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.windows.npz, <prefix>.het_windows.tsv, <prefix>.windows.json and, with --pairs, <prefix>.pair_windows.tsv")
    win.set_defaults(func=snpmatch_windows)

    # not in the reference (its match_insilico_f1s crosses the ten best single accessions): the in-silico F1 of every pair of accessions
    f1s = sub.add_parser('f1search', help="parents of an F1 sample: the in-silico F1 of EVERY pair of accessions of the database scored against the sample")
    f1s.add_argument("-i", "--input_file", dest="inFile", required=True, help="VCF/BED file for the variants in the sample")
    db_options(f1s)
    f1s.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one candidate accession name per line (default: all accessions)")
    f1s.add_argument("--top", dest="top", default=10, type=int, help="pairs of the shortlist, re-scored with the sample's weights (default 10, at most 16)")
    f1s.add_argument("--min_sites", dest="min_sites", default=100, type=int, help="a pair is ranked only with this many informative rows or more (default 100)")
    verbose(f1s)
    f1s.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.f1search.scores.txt, <prefix>.f1search.npz and <prefix>.f1search.json")
    f1s.set_defaults(func=snpmatch_f1search)

    # not in the reference: a contaminated or pooled sample -- reads of two accessions in unequal proportion -- from the allele balance of its reads
    mx = sub.add_parser('mixture', help="a contaminated or pooled sample: the two accessions of the database and the minor fraction that explain the allele depths (FORMAT AD) of the sample best, EVERY ordered pair of accessions tried")
    mx.add_argument("-i", "--input_file", dest="inFile", required=True, help="VCF file of the sample with FORMAT AD (allele depths)")
    db_options(mx)
    mx.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one candidate accession name per line (default: all accessions)")
    mx.add_argument("--bed", dest="bed", default=None, help="use the DB rows of a region only: Chr1,1,1000000 (default: all rows)")
    mx.add_argument("--sites", dest="sitesFile", default=None, help="use the listed rows only: a file with the columns chr and pos (a <prefix>.pruned.tsv of ld, a <prefix>.markers.tsv of markers)")
    mx.add_argument("--sample", dest="sample", default=None, help="sample column of the VCF: its name or its index (default 0)")
    mx.add_argument("--err", dest="err", default=0.01, type=float, help="probability that a read shows the other allele (default 0.01)")
    mx.add_argument("--grid", dest="grid", default=0.01, type=float, help="step of the minor fraction alpha on [0, 0.5]; must divide 0.5 (default 0.01)")
    mx.add_argument("--max_depth", dest="max_depth", default=15, type=int, help="rows with more reads are dropped, 1 .. 255 (default 15)")
    mx.add_argument("--min_reads", dest="min_reads", default=200, type=int, help="an ordered pair is ranked only with this many reads or more on the rows where both are homozygous (default 200)")
    mx.add_argument("--top", dest="top", default=10, type=int, help="ordered pairs of the shortlist (default 10)")
    verbose(mx)
    mx.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.mixture.json, <prefix>.mixture.npz and <prefix>.mixture.scores.txt")
    mx.set_defaults(func=snpmatch_mixture)

    # not in the reference (its cross guesses the parents of an F2 from the single accessions that win clean windows): every pair per window
    par = sub.add_parser('parentsearch', help="parents of a recombinant sample (F2, backcross): EVERY pair of accessions of the database scored per genome window as parent A, parent B or their F1")
    par.add_argument("-i", "--input_file", dest="inFile", required=True, help="VCF/BED file for the variants in the sample")
    db_options(par)
    par.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one candidate accession name per line (default: all accessions)")
    par.add_argument("--genome", dest="genome", default="athaliana_tair10", help="Genome id or path to a reference JSON file (ref_chrs, ref_chrlen)")
    par.add_argument("-b", "--binLength", dest="binLen", default=300000, type=int, help="window length in bp (default 300000)")
    par.add_argument("--top", dest="top", default=10, type=int, help="pairs of the shortlist, with their window tracks (default 10, at most 16)")
    par.add_argument("--min_sites", dest="min_sites", default=100, type=int, help="a pair is ranked only with this many rows or more in its used windows (default 100)")
    par.add_argument("--min_win_sites", dest="min_win_sites", default=5, type=int, help="a window is used for a pair only with this many informative rows or more (default 5)")
    verbose(par)
    par.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.parentsearch.json, <prefix>.parentsearch.npz and <prefix>.parentsearch.windows.tsv")
    par.set_defaults(func=snpmatch_parentsearch)

    # the reference's command, host only: the same draws as the reference under one seed
    sim = sub.add_parser('simulate', help="Given SNP database, check the genotyping efficiency randomly selecting 'n' number of SNPs")
    db_options(sim, required=False)
    sim.add_argument("-a", "--ecotype_id", dest="AccID", help="Ecotype ID you want draw the SNPs")
    sim.add_argument("-n", "--number_of_snps", dest="numSNPs", help="number of SNPs to draw in random to genotype the sample", type=int)
    sim.add_argument("-p", "--error_rate", dest="err_rate", default=0.001, type=float,
                     help="error rate while matching the SNPs, error rate of 0 gives perfect match to the accession")
    sim.add_argument("--f1", action="store_true", dest="simF1", default=False, help="Simulate SNPs for an F1, give parents as 1061x1062 in argument '-a'")
    sim.add_argument("--het_frac", default=1, type=float, dest="rm_het",
                     help="for F1s: the probability that a segregating site stays heterozygous; the rest become homozygous ref or alt, half each")
    sim.add_argument("--seed", dest="seed", default=None, type=int, help="np.random.seed before the draws (not in the reference): the same sample again")
    sim.add_argument("-o", "--output", dest="outFile", help="Output BED file: chromosome, position, genotype")
    verbose(sim)
    sim.set_defaults(func=snpmatch_simulate)

    # not in the reference (simulate + inbred, one accession and one n at a time): every accession simulated and scored against every accession
    pw = sub.add_parser('power', help="identifiability of every accession of the database: with n random SNPs and a call error rate, whom does inbred identify uniquely, whom does it confuse")
    db_options(pw)
    pw.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    pw.add_argument("--bed", dest="bed", default=None, help="draw the markers from the DB rows of a region only: Chr1,1,1000000 (default: all rows)")
    pw.add_argument("--sites", dest="sitesFile", default=None, help="draw the markers from the listed rows only: a file with the columns chr and pos (a <prefix>.sites.tsv of sitestats, a <prefix>.markers.tsv of markers)")
    pw.add_argument("-n", "--number_of_snps", dest="levels", required=True, help="the ladder of marker counts, increasing: 100,1000,10000 (at most 64 levels)")
    pw.add_argument("-p", "--error_rate", dest="err_rate", default=0.001, type=float, help="probability that a call of the simulated sample is redrawn from ref / alt / het (default 0.001)")
    pw.add_argument("--trials", dest="trials", default=3, type=int, help="marker ladders drawn, one device call each (default 3)")
    pw.add_argument("--seed", dest="seed", default=1, type=int, help="seed of the ladders and of the injected errors (default 1)")
    pw.add_argument("--lr_thres", dest="lr_thres", default=3.841, type=float, help="an accession is ambiguous with the top hit below this likelihood ratio (default 3.841, as inbred)")
    verbose(pw)
    pw.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.power.tsv, <prefix>.power.json and <prefix>.power.npz")
    pw.set_defaults(func=snpmatch_power)

    # not in the reference: a sample of more than two sources (MAGIC lines, multi-parent RILs, admixed samples) painted accession by accession
    mos = sub.add_parser('mosaic', help="paint every sample of the input as a mosaic of the accessions of the database: which accession it copies at every matched SNP (copying-model Viterbi with a uniform switch cost)")
    mos.add_argument("-i", "--input_file", dest="inFile", required=True, help="VCF/BED file of the sample; a multi-sample VCF is painted as a batch on its shared records")
    db_options(mos)
    mos.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one candidate accession (founder) name per line (default: all accessions)")
    mos.add_argument("--switch_cost", dest="switch_cost", default=40, type=int, help="cost of a change of accession, 1 .. 1048576 (default 40)")
    mos.add_argument("--mismatch", dest="mismatch", default=2, type=int, help="cost of a homozygous call against the other homozygous call, or against the DB's 'other' code, 0 .. 15 (default 2)")
    mos.add_argument("--het_cost", dest="het_cost", default=1, type=int, help="cost of a heterozygous call against a homozygous one, either way, 0 .. 15 (default 1)")
    mos.add_argument("--min_seg_sites", dest="min_seg_sites", default=20, type=int, help="segments of fewer sites are flagged in the segment table (default 20)")
    verbose(mos)
    mos.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.mosaic.segments.tsv, <prefix>.mosaic.json and <prefix>.mosaic.npz")
    mos.set_defaults(func=snpmatch_mosaic)

    # not in the reference: where along the genome every pair of accessions is identical (shared haplotype segments)
    ibd = sub.add_parser('ibd', help="shared segments (identity by descent): for EVERY pair of accessions of the database the genome windows in which the two are identical, and the runs of such windows along each chromosome")
    db_options(ibd)
    ibd.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    ibd.add_argument("--genome", dest="genome", default="athaliana_tair10", help="Genome id or path to a reference JSON file (ref_chrs, ref_chrlen)")
    ibd.add_argument("-b", "--window_size", dest="binLen", default=100000, type=int, help="window length in bp (default 100000)")
    ibd.add_argument("--min_win_sites", dest="min_win_sites", default=20, type=int, help="a window is used for a pair only with this many rows or more at which both accessions are homozygous (default 20)")
    ibd.add_argument("--max_diff", dest="max_diff", default=0.001, type=float, help="a used window is shared when at most this fraction of those rows differ, 0 .. 1 (default 0.001)")
    ibd.add_argument("--min_run", dest="min_run", default=5, type=int, help="a run is reported with this many shared windows or more (default 5)")
    verbose(ibd)
    ibd.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.ibd.npz, <prefix>.ibd.pairs.tsv, <prefix>.ibd.segments.tsv and <prefix>.ibd.json")
    ibd.set_defaults(func=snpmatch_ibd)

    # not in the reference: a small set of SNPs that separates every pair of accessions (the step after power)
    mks = sub.add_parser('markers', help="a minimal marker set: SNPs chosen greedily so that every pair of accessions of the database differs at --depth of them (homozygous calls only); greedy set cover, not optimal")
    db_options(mks)
    mks.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    mks.add_argument("--bed", dest="bed", default=None, help="candidates: only the DB rows of a region: Chr1,1,1000000 (default: all rows)")
    mks.add_argument("--sites", dest="sitesFile", default=None, help="candidates: only the rows listed in a <prefix>.sites.tsv of sitestats or a <prefix>.pruned.tsv of ld (columns chr and pos)")
    mks.add_argument("--depth", dest="depth", default=1, type=int, help="every pair must differ at this many chosen SNPs, 1 .. 255 (default 1)")
    mks.add_argument("--max_markers", dest="max_markers", default=None, type=int, help="stop after this many SNPs (default: no limit)")
    mks.add_argument("--min_dist_bp", dest="min_dist_bp", default=0, type=int, help="a chosen SNP excludes every candidate closer than this on its chromosome (default 0: no exclusion)")
    verbose(mks)
    mks.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.markers.tsv, <prefix>.markers.json and <prefix>.markers.npz")
    mks.set_defaults(func=snpmatch_markers)

    pc = sub.add_parser('pca', help="population structure of the database: the genotype relationship matrix of its accessions and its principal components; with -i, samples projected onto them")
    db_options(pc)
    pc.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    pc.add_argument("--pops", dest="popFile", default=None, help="text file, accession and population per line: the union of the populations is analysed, every output row carries its population")
    pc.add_argument("--bed", dest="bed", default=None, help="use the DB rows of a region only: Chr1,1,1000000 (default: all rows)")
    pc.add_argument("--sites", dest="sitesFile", default=None, help="use the listed rows only: a file with the columns chr and pos (a <prefix>.pruned.tsv of ld, a <prefix>.sites.tsv of sitestats)")
    pc.add_argument("--min_maf", dest="min_maf", default=0.05, type=float, help="drop rows whose minor allele frequency among the analysed accessions is below this (default 0.05)")
    pc.add_argument("--max_missing", dest="max_missing", default=0.1, type=float, help="drop rows with a larger fraction of missing calls (default 0.1)")
    pc.add_argument("--components", dest="components", default=10, type=int, help="principal components to report, 1 .. min(32, accessions) (default 10)")
    pc.add_argument("--keep_grm", action="store_true", dest="keep_grm", default=False, help="store the relationship matrix in <prefix>.pca.npz")
    pc.add_argument("-i", "--input_file", dest="inFile", default=None, help="samples to project: a VCF (every sample column) or a BED file")
    verbose(pc)
    pc.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.pca.tsv, <prefix>.pca.npz, <prefix>.pca.json and, with -i, <prefix>.projection.tsv")
    pc.set_defaults(func=snpmatch_pca)

    ad = sub.add_parser('admixture', help="ancestry proportions of every accession of the database under the admixture model (K ancestral populations), fitted by EM on the device; writes a --pops file for sitestats / ld / pca; with -i, the proportions of samples")
    db_options(ad)
    ad.add_argument("-a", "--accessions", dest="accFile", default=None, help="text file, one accession name per line (default: all accessions)")
    ad.add_argument("--pops", dest="popFile", default=None, help="text file, accession and population per line: the union of the populations is analysed, the outputs compare the clusters with them")
    ad.add_argument("--bed", dest="bed", default=None, help="use the DB rows of a region only: Chr1,1,1000000 (default: all rows)")
    ad.add_argument("--sites", dest="sitesFile", default=None, help="use the listed rows only: a file with the columns chr and pos (a <prefix>.pruned.tsv of ld, a <prefix>.sites.tsv of sitestats)")
    ad.add_argument("-K", dest="K", required=True, type=int, help="ancestral populations, 1 .. min(16, accessions)")
    ad.add_argument("--min_maf", dest="min_maf", default=0.05, type=float, help="drop rows whose minor allele frequency among the analysed accessions is below this (default 0.05)")
    ad.add_argument("--max_missing", dest="max_missing", default=0.1, type=float, help="drop rows with a larger fraction of missing calls (default 0.1)")
    ad.add_argument("--seed", dest="seed", default=1, type=int, help="restart r starts from numpy.random.default_rng(seed + r) (default 1)")
    ad.add_argument("--restarts", dest="restarts", default=1, type=int, help="runs from different starts; the one with the highest likelihood is reported (default 1)")
    ad.add_argument("--max_iter", dest="max_iter", default=2000, type=int, help="EM iterations per restart, at most (default 2000)")
    ad.add_argument("--tol", dest="tol", default=1e-7, type=float, help="stop when an iteration gains less than this fraction of the log-likelihood (default 1e-7)")
    ad.add_argument("-i", "--input_file", dest="inFile", default=None, help="samples to place: a VCF (every sample column) or a BED file")
    verbose(ad)
    ad.add_argument("-o", "--output", dest="outFile", required=True, help="Output prefix: writes <prefix>.admixture.Q.tsv, .admixture.pops.tsv, .admixture.npz, .admixture.json and, with -i, <prefix>.ancestry.tsv")
    ad.set_defaults(func=snpmatch_admixture)

    mk = sub.add_parser('makedb-native', help="Convert a DB (.npz / HDF5) to the native flat panel format")
    mk.add_argument("-i", "--input", dest="inFile")
    mk.add_argument("-o", "--output", dest="outFile")
    mk.add_argument("--packed", action="store_true", dest="packed", default=False,
                    help="store 2 bits per call (a quarter of the disk and of the bytes a load moves; DBs with the codes -1/0/1/2 only)")
    mk.add_argument("-v", "--verbose", action="store_true", dest="logDebug", default=False)
    mk.set_defaults(func=makedb_native)
    return p


def main(argv=None):
    parser = get_options("SNPmatch inbred / cross scoring on MI355X (snpmatch_amd)", '%(prog)s ' + __version__)
    args = vars(parser.parse_args(argv))
    setLog(args.get('logDebug', False))
    if 'func' not in args:
        parser.print_help()
        return 0
    job = None
    if int(os.environ.get("WORLD_SIZE", "1") or 1) <= 1:
        # a plain CLI run never imports torch (several GPUs are driven through the library's own RCCL group): stay on the
        # HIP runtime the library was built with instead of the copy bundled with a PyTorch wheel
        os.environ.setdefault("SNPMATCH_HIP_RUNTIME", "system")
    try:
        from . import dist
        job = dist.init_from_env()       # under torch.distributed.run: accession-sharded over the ranks' GPUs
        args['func'](args)
        if job is not None:
            import torch.distributed as td
            td.barrier()
            td.destroy_process_group()
        return 0
    except KeyboardInterrupt:
        return 0
    except Exception as e:
        logging.exception(e)
        if job is not None:
            # a rank that fails must not leave its peers waiting in a collective until the launcher's timeout: tear the
            # communicator down (abort where the backend has it) so that their pending calls fail at once
            try:
                import torch.distributed as td
                pg = td.distributed_c10d._get_default_group()
                if hasattr(pg, "abort"):
                    pg.abort()
                else:
                    td.destroy_process_group()
            except Exception:
                pass
        return 2


if __name__ == '__main__':
    sys.exit(main())
