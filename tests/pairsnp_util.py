"""helpers of the pairsnp tests (test infrastructure): the goldens of tests/golden/make_golden_pairsnp.py as files on disk"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["pairsnp_a_plain", "pairsnp_b_phasing", "pairsnp_c_multiallelic", "pairsnp_d_naming", "pairsnp_e_disjoint", "pairsnp_f_db",
         "pairsnp_g_bed"]
DB_NAME = "db.npz"          # the -d argument of the DB case, relative to the directory the case runs in (it is quoted in the JSON)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def bed_text(chrs, pos, gt):
    return "".join("%s\t%d\t%s\n" % (c, p, g) for c, p, g in zip(chrs.tolist(), pos.tolist(), gt.tolist()))


def write_inputs(case, directory):
    """the sample files of a case (named as in the golden) in ``directory``; returns their names (relative to it)"""
    names = case["names"].tolist()
    for k, name in enumerate(names):
        chrs, pos, gt = case["chr_%d" % k], case["pos_%d" % k], case["gt_%d" % k]
        path = os.path.join(directory, name)
        if name.endswith(".bed"):
            with open(path, "w") as fh:
                fh.write(bed_text(chrs, pos, gt))
        else:           # a parser dump, as ``snpmatch parser`` writes it
            np.savez(path, chr=chrs, pos=pos, gt=gt, wei=np.zeros((len(pos), 3)), dp="NA")
    return names


def write_db(case, directory):
    """the DB of a case as a .npz this package loads (positions only matter); None for a case without one"""
    if "db_positions" not in case:
        return None
    n = len(case["db_positions"])
    np.savez(os.path.join(directory, DB_NAME), snps=np.zeros((n, 2), dtype=np.int8), accessions=np.array(["1", "2"], dtype="S"),
             positions=case["db_positions"], chrs=case["db_chrs"].astype("S"), chr_regions=case["db_regions"])
    return DB_NAME


def write_vcf(path, names, chrs, pos, gts):
    """a multi-sample VCF: ``gts`` [n, S] texts"""
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names) + "\n")
        for c, p, row in zip(chrs.tolist(), pos.tolist(), gts.tolist()):
            fh.write("%s\t%d\t.\tA\tT,G\t.\tPASS\t.\tGT\t%s\n" % (c, p, "\t".join(row)))
    return path
