"""
``snpmatch simulate``: draw a test sample from the database -- n random SNPs of one accession (or of the in-silico F1 of two) with call
errors -- as a BED file for ``inbred`` / ``cross``.  Host only; names, arguments and the drawn sample follow the reference module
``snpmatch.core.simulate`` (core/simulate.py:10-68): ``simulateSNPs``, ``simulateSNPs_F1``, ``potatoSimulate``.

Replay.  The functions make the same legacy ``np.random`` calls in the same order as the reference, so under one ``np.random.seed`` they
return the same rows and the same genotypes.  The order is that of Python's evaluation, not of the source text: in
``df.iloc[IDX, 2] = RHS`` the right-hand side is evaluated first, so ``np.random.choice(3, k)`` -- the replacement values -- is drawn
BEFORE the rows they go to, in both functions.  A draw of zero rows is still made: ``choice(..., 0, replace=False)`` shuffles a
permutation and moves the generator on.  The draws come from numpy directly; pandas only carries the returned frame.

Differences from the reference, on purpose:
  * under Python 3 the reference's frame holds bytes (``b'0/0'``) and ``to_csv`` writes ``b'0/0'`` into the bed file, which no reader
    of the reference takes back; here the frame holds str and the file reads ``0/0`` -- what ``ParseInputs`` reads back
  * accession names kept as bytes (the DB files do) are compared as text: the reference's ``AccID in g.g.accessions`` finds no str among
    bytes under Python 3
  * ``--seed`` (the reference has no such flag) calls ``np.random.seed`` first
A DB code other than -1 / 0 / 1 / 2 at a drawn row (``simulateSNPs``) has no text in ``snp_binary_to_gt``: the genotype is the empty
string there, as in the reference's frame (tests/golden/simulate_*.npz show it).

The question ``simulate`` + ``inbred`` answer for one accession and one n is answered for all accessions and a ladder of n by ``power``
(core/power.py), on the device.
"""
import logging

import numpy as np

from . import parsers
from . import snp_genotype

log = logging.getLogger(__name__)


def _names(accessions):
    acc = np.asarray(accessions)
    return np.char.decode(acc, "utf-8") if acc.dtype.kind == "S" else acc.astype("U")


def _frame(chrs, pos, codes):
    """the reference's frame -- columns chr, pos, snp, every cell text (its ``np.column_stack`` of the three makes them so) -- with
    the genotype column as str"""
    import pandas as pd
    gt = parsers.snp_binary_to_gt(codes).astype("U")
    return pd.DataFrame({"chr": np.asarray(chrs).astype("U").astype(object), "pos": np.asarray(pos).astype("U").astype(object),
                         "snp": gt.astype(object)})


def _write(frame, outFile):
    if outFile is not None:
        frame.to_csv(outFile, sep="\t", index=None, header=False)


def simulateSNPs(g, AccID, numSNPs, outFile=None, err_rate=0.001):
    """``numSNPs`` random rows among those where accession ``AccID`` has a call, ``int(err_rate * numSNPs)`` of them redrawn from
    0 / 1 / 2; the frame (chr, pos, snp as GT text), also written to ``outFile`` as a BED file"""
    assert type(AccID) is str, "provide Accession ID as a string"
    names = _names(g.g.accessions)
    assert AccID in names, "accession is not present in the matrix!"
    acc = np.where(names == AccID)[0][0]
    log.info("loading input files")
    acc_snp = np.asarray(g.g_acc.snps[:, acc])
    informative = np.where(acc_snp >= 0)[0]
    chrs, pos = np.array(g.g.chromosomes)[informative], np.asarray(g.g.positions)[informative]
    codes = acc_snp[informative].astype(np.int64)
    log.info("sampling %s positions" % numSNPs)
    drawn = np.sort(np.random.choice(np.arange(len(informative)), numSNPs, replace=False))
    chrs, pos, codes = chrs[drawn], pos[drawn], codes[drawn]
    log.info("adding in error rate: %s" % err_rate)
    num_to_change = int(err_rate * len(codes))
    values = np.random.choice(3, num_to_change)                      # (the right-hand side: drawn first)
    codes[np.sort(np.random.choice(np.arange(len(codes)), num_to_change, replace=False))] = values
    frame = _frame(chrs, pos, codes)
    _write(frame, outFile)
    return frame


def simulateSNPs_F1(g, parents, numSNPs, outFile, err_rate, rm_hets=1):
    """``numSNPs`` random rows among those where both parents (``"6091x6191"``) are homozygous, as their F1: het where they differ.
    ``int(err_rate * numSNPs)`` of the homozygous calls are redrawn from 0 / 1; every het stays het with probability ``rm_hets`` and
    becomes ref or alt with (1 - rm_hets) / 2 each."""
    names = _names(g.g_acc.accessions)
    p1 = np.where(names == parents.split("x")[0])[0][0]
    p2 = np.where(names == parents.split("x")[1])[0][0]
    log.info("loading files!")
    s1, s2 = np.asarray(g.g_acc.snps[:, p1]), np.asarray(g.g_acc.snps[:, p2])
    common = np.where((s1 >= 0) & (s2 >= 0) & (s1 < 2) & (s2 < 2))[0]
    codes = np.where(s1[common] != s2[common], 2, s1[common]).astype(np.int64)
    chrs, pos = np.array(g.g_acc.chromosomes)[common], np.asarray(g.g_acc.positions)[common]
    log.info("sampling %s positions" % numSNPs)
    drawn = np.sort(np.random.choice(np.arange(len(common)), numSNPs, replace=False))
    chrs, pos, codes = chrs[drawn], pos[drawn], codes[drawn]
    log.info("adding in error rate: %s" % err_rate)
    num_to_change = int(err_rate * len(codes))
    values = np.random.choice(2, num_to_change)                      # (the right-hand side: drawn first)
    codes[np.sort(np.random.choice(np.where(codes != 2)[0], num_to_change, replace=False))] = values
    het = np.where(codes == 2)[0]
    codes[het] = np.random.choice(3, het.shape[0], p=[(1 - rm_hets) / 2, (1 - rm_hets) / 2, rm_hets])
    frame = _frame(chrs, pos, codes)
    _write(frame, outFile)
    return frame


def potatoSimulate(args):
    if args.get('seed') is not None:
        np.random.seed(args['seed'])
    g = snp_genotype.Genotype(args['hdf5File'], args['hdf5accFile'])
    if args['simF1']:
        simulateSNPs_F1(g, args['AccID'], args['numSNPs'], args['outFile'], args['err_rate'], args['rm_het'])
    else:
        simulateSNPs(g, args['AccID'], args['numSNPs'], args['outFile'], args['err_rate'])
    log.info("finished!")
