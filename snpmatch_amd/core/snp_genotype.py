"""
DB genotype container (reference: core/snp_genotype.py:24-68,188-211 and the HDF5Genotype duck type of
pygwas/genotype.py:534-673).

``Genotype(hdf5_file, hdf5_acc_file)`` keeps the reference's constructor and the attributes the hot
path uses -- ``g.g.snps[idx, :]``, ``g.g.accessions``, ``g.g.positions``, ``g.g.chrs``,
``g.g.chr_regions``, ``g.g.chromosomes``, ``g.g_acc.snps[:, i]``, ``g.accessions``, ``g.chrs`` -- and
adds ``g.panel(ctx)``: the int8 matrix resident in HBM (uploaded once through the pinned-host staging
path of libsnpmatch_hip), which is what ``Genotyper`` / ``CrossIdentifier`` score against.

On-disk formats
  * native flat panel ``<name>.snpm/``: ``snps.npy`` = int8 [num_snps, num_accessions] C-order (read natively by the
    library's loader threads, streamed to the GPU slab by slab) or ``snps.p2.npy`` = the same matrix with 2 bits per call
    (``save_native(..., packed=True)`` / ``makedb-native --packed``: a quarter of the disk and of the bytes a load moves),
    + ``meta.npz`` (accessions, positions, chrs, chr_regions).
  * ``.npz`` with the same keys plus ``snps`` (small DBs, tests).
  * the reference's HDF5 layout (pygwas/genotype.py:310-326: ``snps`` in lzf chunks of (1000, num_accessions), ``positions``
    with attrs ``chrs`` / ``chr_regions``, ``accessions``), read by the library's own HDF5 reader (``snpmatch_amd.h5``,
    csrc/snpm_h5.cpp) -- h5py is only a fallback for files in formats that reader refuses.
"""
import logging
import os
import re
from glob import glob

import numpy as np

from . import parsers
from .. import _lib

log = logging.getLogger(__name__)
GROUP_MIN_BYTES = 1 << 30          # DBs of at least this many calls are spread over the visible GPUs without being asked to
chunk_size = 1000


class MemGenotype(object):
    """Array-backed stand-in for pygwas HDF5Genotype (attributes used by inbred / cross only)."""

    def __init__(self, snps, accessions, positions, chrs, chr_regions):
        self.snps = snps
        acc = np.asarray(accessions)
        self.accessions = acc if acc.dtype.kind == "S" else np.char.encode(acc.astype("U"), "utf-8")
        self.positions = np.asarray(positions, dtype="i4")
        self.chrs = np.asarray(chrs).astype("U")
        self.chr_regions = np.asarray(chr_regions, dtype=np.int64).reshape(-1, 2)

    @property
    def chromosomes(self):
        """one chromosome name per SNP row (pygwas/genotype.py:156-161), as an array"""
        reps = (self.chr_regions[:, 1] - self.chr_regions[:, 0]).astype(int)
        return np.repeat(self.chrs, reps)

    @property
    def num_snps(self):
        return self.snps.shape[0]


class PackedRows(object):
    """Host view of the 2-bit matrix of a packed flat panel (``snps.p2.npy``: uint8 [n_snp, ceil(n_acc / 4)], field f of byte b =
    accession 4 b + f, 0 ref / 1 alt / 2 het / 3 missing): behaves like the int8 matrix for the reads the host side makes
    (``snps[idx, :]``, ``snps[:, i]``, slices), unpacking what is asked for."""

    def __init__(self, packed, n_acc):
        self.packed, self.shape, self.dtype, self.ndim = packed, (int(packed.shape[0]), int(n_acc)), np.dtype(np.int8), 2

    def __len__(self):
        return self.shape[0]

    @staticmethod
    def unpack(block, n_acc, a0=0):
        """uint8 rows holding accessions a0 .. (a0 % 4 == 0) -> int8 [n, n_acc]"""
        block = np.ascontiguousarray(block)
        fields = (block[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3
        out = fields.reshape(block.shape[0], -1)[:, :n_acc].astype(np.int8)
        out[out == 3] = -1
        return out

    def __getitem__(self, key):
        if not isinstance(key, tuple):
            key = (key, slice(None))
        rows, cols = key
        one_row = isinstance(rows, (int, np.integer))
        block = self.packed[[rows], :] if one_row else self.packed[rows, :]
        if isinstance(cols, (int, np.integer)):
            c = int(cols) + (self.shape[1] if cols < 0 else 0)
            v = ((np.asarray(block[:, c // 4]) >> (2 * (c % 4))) & 3).astype(np.int8)
            v[v == 3] = -1
            return v[0] if one_row else v
        full = self.unpack(block, self.shape[1])[:, cols]
        return full[0] if one_row else full

    def __array__(self, dtype=None, copy=None):
        a = self[:, :]
        return a.astype(dtype) if dtype is not None else a


def save_native(path, snps, accessions, positions, chrs, chr_regions, packed=False):
    """Write the native flat panel directory ``path`` (conventionally ``*.snpm``): ``snps.npy`` (int8 [n_snp, n_acc]) or, with
    ``packed``, ``snps.p2.npy`` (2 bits per call: a quarter of the disk and of the bytes a load moves; only for DBs whose codes
    are -1 / 0 / 1 / 2) plus ``meta.npz``."""
    os.makedirs(path, exist_ok=True)
    n_snp, n_acc = snps.shape
    for stale in ("snps.npy", "snps.p2.npy"):
        if os.path.exists(os.path.join(path, stale)):
            os.remove(os.path.join(path, stale))
    if packed:
        mm = np.lib.format.open_memmap(os.path.join(path, "snps.p2.npy"), mode="w+", dtype=np.uint8, shape=(n_snp, (n_acc + 3) // 4))
        for r0 in range(0, n_snp, 1 << 16):
            mm[r0:r0 + (1 << 16)] = _lib.pack_rows_host(np.asarray(snps[r0:r0 + (1 << 16)]))
    else:
        mm = np.lib.format.open_memmap(os.path.join(path, "snps.npy"), mode="w+", dtype=np.int8, shape=(n_snp, n_acc))
        for r0 in range(0, n_snp, 1 << 16):
            mm[r0:r0 + (1 << 16)] = snps[r0:r0 + (1 << 16)]
    mm.flush()
    del mm
    np.savez(os.path.join(path, "meta.npz"), accessions=np.asarray(accessions).astype("S"),
             positions=np.asarray(positions, dtype="i4"), chrs=np.asarray(chrs).astype("S"),
             chr_regions=np.asarray(chr_regions, dtype=np.int64))


def _load_any(path):
    if os.path.isdir(path):
        meta = np.load(os.path.join(path, "meta.npz"))
        p2 = os.path.join(path, "snps.p2.npy")
        if os.path.exists(p2):                           # packed flat panel: 2 bits per call on disk
            snps = PackedRows(np.load(p2, mmap_mode="r"), len(meta["accessions"]))
            g = MemGenotype(snps, meta["accessions"], meta["positions"], meta["chrs"].astype("U"), meta["chr_regions"])
            g.npy_packed_path = p2
            return g
        snps = np.load(os.path.join(path, "snps.npy"), mmap_mode="r")
        g = MemGenotype(snps, meta["accessions"], meta["positions"], meta["chrs"].astype("U"), meta["chr_regions"])
        g.npy_path = os.path.join(path, "snps.npy")      # lets Genotype.panel() stream the file natively
        return g
    if path.endswith(".npz"):
        d = parsers._StoredNpz.open(path) or np.load(path)       # stored members: views of one memory map (no pass through zipfile)
        return MemGenotype(d["snps"], d["accessions"], d["positions"], np.asarray(d["chrs"]).astype("U"), d["chr_regions"])
    # The reference's HDF5 DB (pygwas/genotype.py:310-326, :534-673): read by the library's own reader (csrc/snpm_h5.cpp) -- no
    # h5py / libhdf5 needed, and the chunks go from the file through the loader's threads into the staging slabs.  Files in a
    # form that reader does not take (unlimited dimensions or more than 8 group members in the "latest" HDF5 file format, other
    # filters) go through h5py where it is installed.
    from .. import h5 as native_h5
    try:
        f = native_h5.File(path)
        g = MemGenotype(f["snps"], f["accessions"][:], f["positions"][:], f["positions"].attrs["chrs"].astype("U"),
                        f["positions"].attrs["chr_regions"])
        g.h5_source = (f, "snps")               # lets Genotype.panel() load rows natively (snpm_panel_load_h5)
        return g
    except IOError as native_error:
        try:
            import h5py
        except ImportError:
            raise IOError("%s; h5py is not installed either -- convert the DB where it is (python -m snpmatch_amd makedb-native)"
                          % native_error)
        h5 = h5py.File(path, "r")
        return MemGenotype(h5["snps"], h5["accessions"][:], h5["positions"][:],
                           h5["positions"].attrs["chrs"].astype("U"), h5["positions"].attrs["chr_regions"])


def load_genotype_files(h5file, hdf5_acc_file=None):
    return Genotype(h5file, hdf5_acc_file)


class Genotype(object):

    def __init__(self, hdf5_file, hdf5_acc_file):
        assert hdf5_file is not None or hdf5_acc_file is not None, "Provide atleast one hdf5 genotype file"
        self._panel = None
        if hdf5_file is None:
            assert os.path.exists(hdf5_acc_file), "Path to %s seems to be broken" % hdf5_acc_file
            self.g_acc = _load_any(hdf5_acc_file)
            return None
        assert os.path.exists(hdf5_file), "Path to %s seems to be broken" % hdf5_file
        self.g = _load_any(hdf5_file)
        if hdf5_acc_file is None:
            hdf5_acc_file = re.sub(r'\.hdf5$', '', hdf5_file) + '.acc.hdf5'
            if len(glob(hdf5_acc_file)) > 0:
                self.g_acc = _load_any(hdf5_acc_file)
            else:
                self.g_acc = self.g        # flat panels serve rows and columns from the same matrix
        else:
            self.g_acc = _load_any(hdf5_acc_file)
        self.accessions = self.g.accessions.astype('U')
        self.chrs = self.g.chrs.astype('U')

    @classmethod
    def from_arrays(cls, snps, accessions, positions, chrs, chr_regions):
        self = cls.__new__(cls)
        self._panel = None
        self.g = MemGenotype(snps, accessions, positions, chrs, chr_regions)
        self.g_acc = self.g
        self.accessions = self.g.accessions.astype('U')
        self.chrs = self.g.chrs.astype('U')
        return self

    # ------------------------------------------------------------------ device residency
    def panel(self, ctx=None, packed=None):
        """The DB matrix resident in HBM (created on first use; slabs go through pinned staging).
        ``packed``: True = 2 bits per call, False = a byte per call, None (default) = environment SNPMATCH_PACKED
        ("1" / "0"; unset or "auto": packed when the DB's codes allow it -- same results bit for bit, a quarter of the HBM and of
        the bytes over PCIe, the scans 2-3 x faster; DBs with codes other than -1/0/1/2 stay int8).
        Where the accession columns live:
          * under ``torch.distributed.run`` (``dist.job()``): this rank's accession shard on this rank's GPU;
          * several GPUs visible to ONE process (SNPMATCH_GPUS, default all): an ``engine.GroupPanel`` -- a shard per
            GPU, results joined by one RCCL all-gather inside the library (no launcher);
          * otherwise: the whole matrix on one GPU."""
        from .. import dist, engine
        if self._panel is None or getattr(self._panel, "h", None) is None:
            if packed is None:
                env = os.environ.get("SNPMATCH_PACKED", "auto").strip().lower()
                packed = None if env in ("", "auto") else env != "0"
            n_acc = len(self.accessions)
            job = dist.job()
            self._shard = job.bounds(n_acc) if job else None
            if self._shard is not None:
                # accession-sharded job (one process per GPU): this rank holds columns [a0, a1) of every SNP row
                assert self._shard[1] > self._shard[0], "more ranks than accession quads: this rank's shard is empty"
                self._panel = self._member_panel(ctx or engine.default_context(), self._shard[0], self._shard[1], packed)
                return self._panel
            group = None
            # several GPUs from one process: when asked for (SNPMATCH_GPUS), or by default for DBs of at least 1 GiB -- below
            # that one GPU loads and scores the DB faster than a communicator is set up
            big = int(self.g.snps.shape[0]) * n_acc >= GROUP_MIN_BYTES
            asked = os.environ.get("SNPMATCH_GPUS", "") != ""
            if ctx is None and (big or asked):
                ids = engine.group_devices()
                if ids is not None:
                    try:
                        group = engine.default_group(engine.GroupPanel.usable_members(n_acc, len(ids)))
                    except (RuntimeError, OSError) as e:
                        # several GPUs were found but their communicator could not be formed (RCCL missing or unable to reach
                        # a peer): a job that did not ask for them runs on one GPU, a job that did is told
                        if asked:
                            raise
                        log.warning("the %d visible GPUs cannot form a group (%s): using one GPU", len(ids), e)
                        group = None
            if group is not None:
                self._panel = engine.GroupPanel.build(group, n_acc, lambda c, a0, a1: self._member_panel(c, a0, a1, packed))
            else:
                self._panel = self._member_panel(ctx or engine.default_context(), 0, n_acc, packed)
        return self._panel

    def _member_panel(self, ctx, a0, a1, packed):
        """Columns [a0, a1) of the DB on one GPU, planned by the HBM the GPU has free (SNPM_HBM_BUDGET_GB overrides; 1 GB =
        1e9 bytes): the int8 matrix whole -> the 2-bit packed matrix whole (same results, a quarter of the bytes; DBs with
        call codes other than -1/0/1/2 cannot take this step) -> SNP slabs streamed from the file / array through two
        half-buffers (``engine.StreamedPanel``; the reference reads any size through g.g.snps[idx, :])."""
        from .. import engine
        npy = getattr(self.g, "npy_path", None)          # native flat panel: file -> pinned slabs -> HBM
        h5_source = getattr(self.g, "h5_source", None)   # the reference's HDF5 file: chunks -> loader threads -> pinned slabs -> HBM
        p2 = getattr(self.g, "npy_packed_path", None)    # packed flat panel: the file's 2-bit rows travel as they are
        store = (engine.RowStore(npy=npy) if npy else engine.RowStore(npy_packed=(p2, len(self.accessions))) if p2
                 else engine.RowStore(h5=h5_source) if h5_source else engine.RowStore(snps=self.g.snps))
        env = os.environ.get("SNPM_HBM_BUDGET_GB", "")
        budget = int(float(env) * 1e9) if env else int(0.85 * ctx.mem_info()[0])
        n_loc = a1 - a0

        def need(pk):
            return (store.n_snp + 32) * ctx.row_pitch(n_loc, pk) + 256

        # packed None (auto): the packed panel first -- it loads faster (a quarter of the bytes cross PCIe, packed by the host
        # threads) and scans faster -- then int8; False: int8 first, packed only when int8 does not fit; True: packed
        unpackable = False
        for pk in ([True, False] if packed is None else [True] if packed else [False, True]):
            if need(pk) > budget:
                continue
            try:
                return engine.Panel.from_store(ctx, store, packed=pk, cols=(a0, a1))
            except AssertionError:
                if not pk:
                    raise
                log.info("DB holds codes a packed panel cannot store; using the int8 panel")
                unpackable = True
                if packed and need(False) <= budget:
                    return engine.Panel.from_store(ctx, store, packed=False, cols=(a0, a1))
        log.info("DB shard of %.1f GB does not fit the HBM budget of %.1f GB: streaming SNP slabs", need(False) / 1e9, budget / 1e9)
        # slabs: packed when asked for, or when the file itself is packed; in auto mode an int8 source streams as int8 (a call
        # code a packed panel refuses could otherwise surface in the middle of a job, slabs after the first are not probed)
        if (packed or (packed is None and p2)) and not unpackable:
            sp = None
            try:
                sp = engine.StreamedPanel(ctx, store, cols=(a0, a1), packed=True, budget_bytes=budget)
                sp.store.load(sp.halves[0], sp.cols, (0, min(sp.rows_cap, store.n_snp)), 0)     # probe for codes a packed panel refuses
                return sp
            except AssertionError as e:
                # (the constructor itself asserts when the budget holds no row: then there is nothing to free)
                log.info("packed slabs not usable (%s); streaming int8 slabs", e)
                if sp is not None:
                    sp.free()
        return engine.StreamedPanel(ctx, store, cols=(a0, a1), packed=False, budget_bytes=budget)

    # ------------------------------------------------------------------ position intersection (a5)
    def _region_is_increasing(self, ci, pos):
        """DB positions of chromosome ``ci`` strictly increasing?  (checked once per DB object)"""
        cache = self.__dict__.setdefault("_increasing_regions", {})
        if ci not in cache:
            cache[ci] = bool(len(pos) < 2 or np.all(pos[1:] > pos[:-1]))
        return cache[ci]

    def get_positions_idxs(self, commonSNPsCHR, commonSNPsPOS, _parsed=None):
        """(db_row_idx, sample_idx) of the positions present in both; core/snp_genotype.py:43-44.
        Same result as ``get_common_positions(chromosomes, positions, ...)`` without materialising one
        chromosome string per DB row: the DB side is walked region by region (pygwas chr_regions).
        ``_parsed``: the ``ParseInputs`` these arrays belong to, when its chromosome names are already filtered
        (``Genotyper`` / ``CrossIdentifier`` call ``filter_chr_names`` on construction): nothing is copied or re-derived."""
        if _parsed is not None and getattr(_parsed, "g_chr_codes", None) is not None and len(_parsed.g_chr_codes) == len(commonSNPsPOS):
            ins = _parsed
        else:
            ins = parsers.ParseInputs("")
            ins.load_snp_info(snpCHR=commonSNPsCHR, snpPOS=commonSNPsPOS, snpGT="", snpWEI=np.nan, DPmean=0)
            ins.filter_chr_names()
        db_ids = self.__dict__.get("_db_chr_ids")
        if db_ids is None:                       # once per DB object
            db_ids = self._db_chr_ids = np.array([re.sub("chr", "", c, flags=re.IGNORECASE) for c in self.g.chrs.astype("U").tolist()], dtype="str")
        sample_ids = ins.g_chrs_ids.tolist()
        sample_pos = np.ascontiguousarray(ins.pos, dtype=np.int64)
        positions = self.__dict__.get("_positions_i64")
        if positions is None:                    # one int64 copy per DB object (HDF5 stores int32)
            positions = self._positions_i64 = np.ascontiguousarray(self.g.positions, dtype=np.int64)
        regions = np.asarray(self.g.chr_regions)
        idx1 = [np.zeros(0, dtype=int)]
        idx2 = [np.zeros(0, dtype=int)]
        seen = set()
        for ci, cid in enumerate(db_ids):
            if cid in seen:             # a chromosome id listed twice: fall back to the generic path
                return self.get_common_positions(self.g.chromosomes, positions, commonSNPsCHR, commonSNPsPOS)
            seen.add(cid)
            if regions[ci][1] <= regions[ci][0] or cid not in ins.g_chrs_ids:
                continue
            s, e = int(regions[ci][0]), int(regions[ci][1])
            ix2 = np.flatnonzero(ins.g_chr_codes == sample_ids.index(cid))
            p1 = positions[s:e]
            if len(ix2) and ix2[-1] - ix2[0] + 1 == len(ix2):       # one run of the sorted input: a view, no gather
                p2 = sample_pos[ix2[0]:ix2[-1] + 1]
            else:
                p2 = sample_pos[ix2]
            # native sorted merge (strictly increasing inputs); the DB side is verified once per chromosome, after
            # which a short sample list is located by galloping search instead of a walk over every DB position
            merged = _lib.intersect_sorted(p1, p2, a_verified=self._region_is_increasing(ci, p1))
            if merged is not None:
                idx1.append(s + merged[0])
                idx2.append(ix2[merged[1]])
            else:                                           # the reference's np.in1d pair, quirks included
                idx1.append(s + np.where(np.isin(p1, p2, assume_unique=True))[0])
                idx2.append(ix2[np.where(np.isin(p2, p1, assume_unique=True))[0]])
        return (np.concatenate(idx1).astype(int), np.concatenate(idx2).astype(int))

    @staticmethod
    def get_common_positions(input_1_chr, input_1_pos, input_2_chr, input_2_pos):
        """Rows of input 1 and of input 2 whose (chromosome, position) occurs in both, chromosomes in the order in
        which input 1 first names them (the contract of core/snp_genotype.py:46-68; 'Chr1' / 'chr1' / '1' are one
        chromosome).  Each side is grouped once (one stable sort of its chromosome index); a chromosome both sides
        hold is intersected by the native sorted merge when both position lists are strictly increasing, otherwise by
        the membership masks the reference builds (np.isin with assume_unique, quirks on repeated positions included)."""
        assert len(input_1_chr) == len(input_1_pos), "Both chromosome and position array provided should be of same length"
        assert len(input_2_chr) == len(input_2_pos), "Both chromosome and position array provided should be of same length"
        side1, side2 = _rows_by_chromosome(input_1_chr, input_1_pos), _rows_by_chromosome(input_2_chr, input_2_pos)
        hits1, hits2 = [np.zeros(0, dtype=int)], [np.zeros(0, dtype=int)]
        for cid in side1.order:
            if cid not in side2.rows:
                continue
            rows1, rows2 = side1.rows[cid], side2.rows[cid]
            pos1, pos2 = side1.pos[rows1], side2.pos[rows2]
            merged = _lib.intersect_sorted(pos1, pos2)
            if merged is not None:
                hits1.append(rows1[merged[0]])
                hits2.append(rows2[merged[1]])
            else:
                hits1.append(rows1[np.isin(pos1, pos2, assume_unique=True)])
                hits2.append(rows2[np.isin(pos2, pos1, assume_unique=True)])
        return (np.concatenate(hits1).astype(int), np.concatenate(hits2).astype(int))

    def get_matching_accs_ix(self, accs, return_np=False):
        acc_ix = []
        for ea in accs:
            t_ix = np.where(self.accessions == ea)[0]
            acc_ix.append(None if len(t_ix) == 0 else t_ix[0])
        if return_np:
            acc_ix = np.array([a for a in acc_ix if a is not None], dtype="int")
        return acc_ix

    # ------------------------------------------------------------------ regions and relatedness
    def get_chr_ind(self, echr):
        """Which of the DB's chromosomes ``echr`` names ('Chr1', 'chr1' and '1' are one chromosome): its index, or None when
        no chromosome, or more than one, carries that id."""
        wanted = _bare_chr_id(echr)
        matches = [k for k, name in enumerate(self.chrs.tolist()) if _bare_chr_id(name) == wanted]
        return matches[0] if len(matches) == 1 else None

    def determine_snp_ix_given_bed(self, req_bed):
        """DB rows inside a region given as ``"Chr1,1,1000"`` or as a (chromosome, start, end) triple: the consecutive rows of
        that chromosome from the first position >= start up to, not including, the first position >= end."""
        fields = [f.strip() for f in req_bed.split(",")] if isinstance(req_bed, str) else list(req_bed)
        if len(fields) != 3:
            raise ValueError("a region is chromosome,start,end (Chr1,1,1000000): got %r" % (req_bed,))
        name, lo, hi = fields[0], int(fields[1]), int(fields[2])
        which = self.get_chr_ind(name)
        assert which is not None, "chromosome %s is not in the database" % name
        first, last = (int(v) for v in np.asarray(self.g.chr_regions)[which])
        bounds = np.searchsorted(np.asarray(self.g.positions[first:last]), [lo, hi], side="left")
        return np.arange(first + int(bounds[0]), first + int(bounds[1]))

    def kinship_counts(self, filter_acc_ix=None, filter_snp_ix=None):
        """(ninfo, same, diff) int32 [n, n] of the listed accessions over the listed DB rows, counted on the resident panel
        (``engine.kinship_counts``): rows where both calls are informative, where both are homozygous and equal, where both are
        homozygous and different.  None = all accessions / all rows; a row list that is a run ``r, r + 1, ...`` is scanned as a
        dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "kinship needs", filter_snp_ix)
        return engine.kinship_counts(panel, filter_acc_ix, rows)

    def kinship_given_snps(self, filter_acc_ix=None, filter_snp_ix=None):
        """Kinship between all pairs of the listed accessions over the listed DB rows (core/snp_genotype.py:256-289): fp64 ndarray
        ``(same - diff) / ninfo``, ``nan`` where a pair shares no informative row.  The reference sums ``calc_kinship_mat`` over
        1000-row chunks -- sums of integers in fp64, exact -- and divides once: one division of the same two integers gives its
        bits.  Two places where its method cannot be followed: with ``filter_acc_ix=None`` it indexes with ``[:, None]`` and fails
        (here: all accessions); its line 272 replaces a given ``filter_snp_ix`` by ``arange(len)``, i.e. uses the FIRST ``len``
        rows (here: the listed rows)."""
        ninfo, same, diff = self.kinship_counts(filter_acc_ix, filter_snp_ix)
        return kinship_from_counts(ninfo, same, diff)

    def f1_counts(self, sample_class, filter_acc_ix=None, filter_snp_ix=None):
        """(hits, ninfo) int32 [n, n] of the in-silico F1 of every pair of the listed accessions against a sample's hard calls
        over the listed DB rows, counted on the resident panel (``engine.f1_counts``).  ``sample_class``: uint8, one class per
        listed row (0 ref, 1 alt, 2 het, 0xFF none).  None = all accessions / all rows; a row list that is a run ``r, r + 1, ...``
        is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the exhaustive F1 search needs", filter_snp_ix)
        return engine.f1_counts(panel, sample_class, filter_acc_ix, rows)

    def mix_counts(self, alt, ref, filter_acc_ix=None, filter_snp_ix=None):
        """int32 [2, 2, 2, n, n]: for every ordered pair of the listed accessions the sample's alt and ref reads summed over the
        listed DB rows by the pair's two homozygous calls, on the resident panel (``engine.mix_counts``).  ``alt`` / ``ref``: one
        read count (0 .. 255) per listed row.  None = all accessions / all rows; a row list that is a run ``r, r + 1, ...`` is
        scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the mixture scan needs", filter_snp_ix)
        return engine.mix_counts(panel, alt, ref, filter_acc_ix, rows)

    def parent_counts(self, sample_class, win_off, min_win_sites=1, filter_acc_ix=None, filter_snp_ix=None):
        """(score, n_tot, w_first, w_het) int32 [n, n] of every pair of the listed accessions taken, window by window, as the parents
        of a recombinant sample, over the listed DB rows grouped into windows by ``win_off``, counted on the resident panel
        (``engine.parent_counts``).  ``sample_class``: uint8, one class per listed row (0 ref, 1 alt, 2 het, 0xFF none).  None = all
        accessions / all rows; a row list that is a run ``r, r + 1, ...`` is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the parent search needs", filter_snp_ix)
        return engine.parent_counts(panel, sample_class, win_off, min_win_sites, filter_acc_ix, rows)

    def ibd_counts(self, win_off, min_win_sites=20, max_diff_ppm=1000, min_run=1, filter_acc_ix=None, filter_snp_ix=None, bits=True):
        """the dict of ``engine.ibd_counts`` -- w_used, w_shared, n_shared, d_shared, run_max, n_runs, w_in_runs int32 [n, n] and the
        used / shared window bitsets -- of every pair of the listed accessions over the listed DB rows grouped into windows by
        ``win_off``, counted on the resident panel: the windows in which two accessions are identical and the runs they form.  None
        = all accessions / all rows; ``filter_snp_ix`` may be a ``range``; a row list that is a run ``r, r + 1, ...`` is scanned as
        a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the shared-segment scan needs", filter_snp_ix)
        return engine.ibd_counts(panel, win_off, min_win_sites, max_diff_ppm, min_run, filter_acc_ix, rows, bits)

    def marker_select(self, depth=1, max_markers=None, coord=None, min_dist=0, eligible=None, filter_acc_ix=None, filter_snp_ix=None, first_gain=True):
        """the dict of ``engine.marker_select`` -- chosen, gain_at, n_chosen, remaining, stop_reason, need, first_gain -- of the greedy
        choice of DB rows that separate every pair of the listed accessions ``depth`` times, made on the resident panel; positions
        are indices into the listed rows.  None = all accessions / all rows; ``filter_snp_ix`` may be a ``range``; a row list that is
        a run ``r, r + 1, ...`` is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the marker selection needs", filter_snp_ix)
        return engine.marker_select(panel, depth, max_markers, coord, min_dist, eligible, filter_acc_ix, rows, first_gain)

    def gram(self, tab, filter_acc_ix=None, filter_snp_ix=None):
        """fp64 [n, n]: the Gram matrix ``sum_s t(s, i) t(s, j)`` of the listed accessions over the listed DB rows, made on the
        resident panel (``engine.gram``).  ``tab``: fp64 [rows, 4], the value of a call with code 0 / 1 / 2 / 3 per listed row; a
        missing call has value 0.  None = all accessions / all rows; ``filter_snp_ix`` may be a ``range``; a row list that is a run
        ``r, r + 1, ...`` is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the principal component analysis needs", filter_snp_ix)
        return engine.gram(panel, tab, filter_acc_ix, rows)

    def loadings(self, tab, vec, filter_acc_ix=None, filter_snp_ix=None):
        """fp64 [rows, k]: ``sum_i t(s, i) vec[i, c]`` over the listed accessions for every listed DB row, made on the resident
        panel (``engine.loadings``).  ``tab`` / ``filter_acc_ix`` / ``filter_snp_ix`` as for ``gram``; ``vec``: fp64 [n, k]."""
        from .. import engine
        panel, rows = _scan_of(self, "the principal component analysis needs", filter_snp_ix)
        return engine.loadings(panel, tab, vec, filter_acc_ix, rows)

    def admix(self, Q, F, n_iter=1, filter_acc_ix=None, filter_snp_ix=None, update_q=True, update_f=True):
        """(Q, F, loglik) after ``n_iter`` joint EM iterations of the admixture model on the listed accessions over the listed DB
        rows, made on the resident panel (``engine.admix``).  ``Q``: fp64 [n, K]; ``F``: fp64 [rows, K]; ``filter_acc_ix`` /
        ``filter_snp_ix`` as for ``gram``."""
        from .. import engine
        panel, rows = _scan_of(self, "the admixture model needs", filter_snp_ix)
        return engine.admix(panel, Q, F, n_iter, filter_acc_ix, rows, update_q, update_f)

    def sim_counts(self, grp_off, err_rate, seed, filter_acc_ix=None, filter_snp_ix=None):
        """(score, ninfo) int32 [n_grp, n, n] of the sample simulated from every listed accession (its calls at the listed DB rows,
        errors at ``err_rate`` injected under ``seed``) against every listed accession, per group of the listed rows as ``grp_off``
        cuts them, counted on the resident panel (``engine.sim_counts``).  Row a is the sample, column b the DB accession.  None = all
        accessions / all rows; a row list that is a run ``r, r + 1, ...`` is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the power study needs", filter_snp_ix)
        return engine.sim_counts(panel, grp_off, err_rate, seed, filter_acc_ix, rows)

    def mosaic(self, classes, chain_off, cost, switch_cost, filter_acc_ix=None, filter_snp_ix=None, want_col_cost=False):
        """(state, chain_cost, col_cost) of the samples painted as mosaics of the listed accessions over the listed DB rows, which
        ``chain_off`` cuts into chains (``engine.mosaic``: the copying-model Viterbi on the resident panel).  ``classes``: uint8
        [n_samples, n_rows], one class per sample and listed row (0 ref, 1 alt, 2 het, 0xFF none).  None = all accessions / all
        rows; a row list that is a run ``r, r + 1, ...`` is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "the mosaic needs", filter_snp_ix)
        return engine.mosaic(panel, classes, chain_off, cost, switch_cost, filter_acc_ix, rows, want_col_cost)

    # ------------------------------------------------------------------ site statistics
    def site_counts(self, filter_acc_ix=None, filter_snps_ix=None):
        """int32 [G, n, 4] -- c0, c1, c2 (listed accessions with code 0 / 1 / 2) and ninfo (listed accessions with a call) of every
        listed DB row, counted on the resident panel in one pass (``engine.site_counts``).  ``filter_acc_ix``: None (all accessions,
        G = 1), an index array (G = 1; a repeat counts as listed) or a dict name -> index array (G = len(dict), in the dict's
        order).  ``filter_snps_ix``: None = all rows; a row list that is a run ``r, r + 1, ...`` is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "site statistics need", filter_snps_ix)
        if isinstance(filter_acc_ix, dict):
            for name, ix in filter_acc_ix.items():
                assert type(ix) is np.ndarray, "provide numpy arrays in a dictionary when giving subpopulations (%r)" % (name,)
            groups = [filter_acc_ix[name] for name in filter_acc_ix]
        else:
            groups = None if filter_acc_ix is None else [np.asarray(filter_acc_ix).reshape(-1)]
        return engine.site_counts(panel, groups, rows)

    def get_af_snps(self, no_accs_missing_info, return_nind=False, filter_snps_ix=None, filter_acc_ix=None, polarize_geno=1, return_maf=True):
        """Allele frequency of the listed DB rows among the listed accessions (core/snp_genotype.py:119-175): fp64
        ``(2 * #polarize_geno + #het) / (2 * #informative)``, ``nan`` where no more than ``no_accs_missing_info`` listed
        accessions carry a call; with ``return_maf`` the smaller of it and its complement.  ``return_nind``: also the number of
        informative accessions per row (int64).  ``filter_acc_ix`` as a dict name -> index array gives dicts name -> fp64 array for
        both (the reference appends its counts to a float array there).  The reference walks 1000-row chunks and gathers the panel
        once per subpopulation; here every listed row is read once on the device for all of them and the division is made once
        per row from the same two integers.  One place where its semantics are the panel's and not numpy's: a call is missing
        when it is negative (the reference tests ``== -1``; a panel stores every missing call as -1)."""
        counts = self.site_counts(filter_acc_ix, filter_snps_ix)
        if isinstance(filter_acc_ix, dict):
            maf = {name: af_from_counts(counts[k], no_accs_missing_info, polarize_geno, return_maf) for k, name in enumerate(filter_acc_ix)}
            nind = {name: counts[k, :, 3].astype(np.float64) for k, name in enumerate(filter_acc_ix)}
        else:
            maf = af_from_counts(counts[0], no_accs_missing_info, polarize_geno, return_maf)
            nind = counts[0, :, 3].astype(np.int64)
        return (maf, nind) if return_nind else maf

    def polarize_mask(self, filter_acc_ix=None, filter_snps_ix=None, polarize_geno=1):
        """bool [n]: the listed DB rows that ``_polarize_snps`` of the reference would flip when given the listed accessions --
        those where more than half of the LISTED accessions (a repeat counts as listed, missing calls count in the half) carry
        ``polarize_geno`` -- from the device counts."""
        if polarize_geno not in (0, 1, 2):
            raise ValueError("polarize_geno must be 0, 1 or 2, got %r" % (polarize_geno,))
        if isinstance(filter_acc_ix, dict):
            raise TypeError("polarize_mask takes one accession list (or None), not a dict of subpopulations")
        n_listed = len(self.accessions) if filter_acc_ix is None else np.asarray(filter_acc_ix).size
        counts = self.site_counts(filter_acc_ix, filter_snps_ix)
        return counts[0, :, int(polarize_geno)] > float(n_listed) / 2

    # ------------------------------------------------------------------ linkage disequilibrium
    def ld_band(self, band, filter_acc_ix=None, filter_snps_ix=None, v_alt=2, v_het=1, min_n=2, counts=True, r2=True):
        """``(counts, r2)`` of every listed DB row with each of the ``band`` listed rows after it, among the listed accessions,
        computed on the resident panel in one call (``engine.ld_band``): int32 [n, band, 9] -- n, Ak, Hk, Aj, Hj, AA, AH, HA, HH --
        and fp64 [n, band] (``ld_from_counts`` of them).  ``filter_acc_ix``: None = all accessions, else DISTINCT indices;
        ``filter_snps_ix``: None = all rows; a row list that is a run ``r, r + 1, ...`` is scanned as a dense range."""
        from .. import engine
        panel, rows = _scan_of(self, "LD needs", filter_snps_ix)
        return engine.ld_band(panel, band, filter_acc_ix, rows, v_alt, v_het, min_n, counts, r2)

    def calculate_ld(self, snp_ix, accs_ix=None, v_alt=2, v_het=1, min_n=2):
        """The full symmetric r2 matrix, fp64 [n, n], of the listed DB rows among the listed accessions (core/snp_genotype.py:291-295
        names it: the method there indexes the wrong axis and writes ``nan`` into an int8 array).  Built from ONE band call with
        ``band = n - 1`` -- cell [k][d - 1] is the pair (k, k + d) -- and one ``site_counts`` call for the diagonal: 1, or nan
        for a row that is constant among its informative accessions (or has fewer than ``min_n`` of them).  A missing call leaves
        the PAIR's sum, not the whole matrix, as it would in the dense form.  Lists longer than ``engine.LD_MAX_BAND + 1`` rows are
        refused: a dense matrix is the wrong shape for them, ``ld_band`` gives the band."""
        from .. import engine
        snp_ix = np.asarray(snp_ix, dtype=np.int64).reshape(-1)
        n = len(snp_ix)
        if n - 1 > engine.LD_MAX_BAND:
            raise ValueError("calculate_ld builds a dense matrix from one band call and takes at most %d rows, got %d: ask ld_band "
                             "for the band of a longer list" % (engine.LD_MAX_BAND + 1, n))
        out = np.full((n, n), np.nan, dtype=np.float64)
        if n == 0:
            return out
        site = self.site_counts(accs_ix, snp_ix)[0].astype(np.int64)
        own = np.zeros((n, 9), dtype=np.int64)                      # a row paired with itself
        own[:, 0] = site[:, 0] + site[:, 1] + site[:, 2]
        own[:, 1] = own[:, 3] = own[:, 5] = site[:, 1]
        own[:, 2] = own[:, 4] = own[:, 8] = site[:, 2]
        out[np.arange(n), np.arange(n)] = ld_from_counts(own, v_alt, v_het, min_n)
        if n > 1:
            band = self.ld_band(n - 1, accs_ix, snp_ix, v_alt, v_het, min_n, counts=False)[1]
            for d in range(1, n):
                k = np.arange(n - d)
                out[k, k + d] = out[k + d, k] = band[:n - d, d - 1]
        return out

    # ------------------------------------------------------------------ genome windows
    def window_counts(self, win_off, filter_acc_ix=None, pairs=None, filter_snps_ix=None, acc_counts=True):
        """``(acc, pair)`` per window of the listed DB rows, counted on the resident panel in one call (``engine.window_counts``):
        int32 [n_win, n_acc, 4] -- c0, c1, c2, ninfo of every listed accession -- and int32 [n_pairs, n_win, 4] -- n, eq, hom_same,
        hom_diff of every listed pair.  ``win_off`` [n_win + 1] cuts the LISTED rows into windows; ``pairs`` [n_pairs, 2] indexes
        the accession list.  ``filter_snps_ix``: None = all rows, a ``range``, or a row list (a run ``r, r + 1, ...`` is scanned as
        a dense range)."""
        from .. import engine
        panel, rows = _scan_of(self, "window counts need", filter_snps_ix)
        return engine.window_counts(panel, win_off, filter_acc_ix, pairs, rows, acc_counts)

    def genome_window_counts(self, genome_class, window_size, filter_acc_ix=None, pairs=None, acc_counts=True):
        """The same over the windows of a genome (``Genome.get_window_rows``): ``((chr_ix, start, end, first, last), acc, pair)``
        with one device call per chromosome, whose rows are a range.  A window without rows keeps zero counts."""
        table = genome_class.get_window_rows(self.g, window_size)
        chr_ix, first, last = table[0], table[3], table[4]
        n_win = len(chr_ix)
        n_acc = len(self.accessions) if filter_acc_ix is None else np.asarray(filter_acc_ix).size
        acc = np.zeros((n_win, n_acc, 4), dtype=np.int32) if acc_counts else None
        pair = None if pairs is None else np.zeros((len(np.asarray(pairs).reshape(-1, 2)), n_win, 4), dtype=np.int32)
        for c in range(len(genome_class.chrs)):
            w = np.flatnonzero(chr_ix == c)
            if not len(w) or last[w[-1]] <= first[w[0]]:
                continue
            r0, r1 = int(first[w[0]]), int(last[w[-1]])
            got_a, got_p = self.window_counts(np.append(first[w], r1) - r0, filter_acc_ix, pairs, range(r0, r1), acc_counts)
            if acc_counts:
                acc[w] = got_a
            if pairs is not None:
                pair[:, w] = got_p
        return table, acc, pair

    def calculate_heterozygosity_windows(self, genome_class, window_size, sample_ix=None):
        """Called heterozygosity of the listed accessions in the windows of a genome (core/snp_genotype.py:332-345): a frame indexed
        ``Chr1,1,300000``, one fp64 column per entry of ``sample_ix`` (None: all accessions), ``#het / #informative`` of the window's
        rows, ``nan`` where no more than 5 rows are informative.  As in the reference the denominator counts every call >= 0, an
        int8 DB's code 3 included.  The reference gathers the panel once per window; here the rows of a chromosome are read once on
        the device for all its windows and the division is made once per cell from the same two integers."""
        import pandas as pd
        from . import genomes
        assert type(genome_class) is genomes.Genome, "provide a genome class, snpmatch.genomes.Genome"
        if sample_ix is None:
            sample_ix = np.arange(len(self.accessions))
        sample_ix = np.asarray(sample_ix).reshape(-1)
        (chr_ix, start, end, _, _), acc, _ = self.genome_window_counts(genome_class, window_size, sample_ix)
        beds = ["%s,%d,%d" % (genome_class.chrs[c], s, e) for c, s, e in zip(chr_ix.tolist(), start.tolist(), end.tolist())]
        return pd.DataFrame(het_from_counts(acc, 5), index=beds, columns=sample_ix, dtype=float)

    def mismatch_between_accs(self, acc_x_ix, acc_y_ix, bin_length=None, genome_class=None):
        """Where two accessions differ (core/snp_genotype.py:297-330).  Without ``bin_length``: fp64 [n_snps], 1 where the two calls
        are equal, 0 where they differ, ``nan`` where either is missing or above 2 -- host work on the two columns.  With
        ``bin_length`` and a ``Genome``: a frame chr / start / end / mismatch, one row per window of the genome, ``mismatch = 1 -
        #equal / #both called`` (``nan`` for a window where the two share no call), counted on the resident panel.  The reference
        reads the column-chunked file here; both forms use the same matrix."""
        if bin_length is None:
            snps = self.g_acc.snps
            x, y = (np.asarray(snps[:, int(ix)]).astype(np.int64).reshape(-1) for ix in (acc_x_ix, acc_y_ix))
            out = (x == y).astype(np.float64)
            out[(x < 0) | (x > 2) | (y < 0) | (y > 2)] = np.nan
            return out
        import pandas as pd
        from . import genomes
        assert type(bin_length) is int, "provide an interger for window length"
        assert type(genome_class) is genomes.Genome, "provide genome class to determine windows in genome"
        (chr_ix, start, end, _, _), _, pair = self.genome_window_counts(genome_class, bin_length, np.array([int(acc_x_ix), int(acc_y_ix)]),
                                                                        [[0, 1]], acc_counts=False)
        frame = pd.DataFrame({'chr': np.asarray(genome_class.chrs)[chr_ix].astype(object), 'start': start.astype(object), 'end': end.astype(object),
                              'mismatch': mismatch_from_counts(pair[0]).astype(object)}, columns=['chr', 'start', 'end', 'mismatch'])
        return frame

    # ------------------------------------------------------------------ --refine support
    def identify_segregating_snps(self, accs_ix):
        """DB rows where the given accessions do not all carry the same informative call
        (core/snp_genotype.py:188-211, segregting_snps :378-383) -- scanned on the device, where the DB lives."""
        mask = self.segregating_mask(accs_ix)
        return None if mask is None else np.where(mask)[0]

    def segregating_mask(self, accs_ix):
        """the same as a mask over the DB rows (what ``Genotyper.filter_tophits`` indexes with its matched rows: turning 11M
        flags into 7M indices and testing 200k rows against them cost 50 ms of a --refine run, the scan itself 1 ms)"""
        assert type(accs_ix) is np.ndarray, "provide an np array for list of indices to be considered"
        assert len(accs_ix) > 1, "polymorphism happens in more than 1 line"
        if len(accs_ix) > (len(self.accessions) / 2):
            return None
        panel = self.panel()                       # resident after the genome-wide pass; uploaded now otherwise
        shard = getattr(self, "_shard", None)      # (a GroupPanel combines its members' scans itself)
        if shard is not None:
            # accession-sharded: every rank scans the listed accessions it holds; a row segregates when some
            # rank saw two different calls, or two ranks saw different ones
            from .. import dist
            accs_ix = np.asarray(accs_ix)
            local = accs_ix[(accs_ix >= shard[0]) & (accs_ix < shard[1])] - shard[0]
            mask, first = panel.segregating_first(local)
            both = dist.job().all_gather_bytes(np.stack([mask, first]))          # [world, 2, n_snp]
            firsts = both[:, 1, :]
            seen = firsts != 0xFF
            lo = np.where(seen, firsts, 255).min(axis=0)
            hi = np.where(seen, firsts, 0).max(axis=0)
            return both[:, 0, :].any(axis=0) | (seen.any(axis=0) & (lo != hi))
        return panel.segregating_rows(accs_ix)                      # one device scan over the listed columns (k_segregating)


def _resident_panel(g, who_needs):
    """the panel of a ``Genotype`` for a scan that needs every accession column on one device (kinship, site statistics, LD):
    accession-sharded and streamed DBs are refused with the reason"""
    from .. import engine
    panel = g.panel()
    if getattr(g, "_shard", None) is not None or not isinstance(panel, engine.Panel):
        raise TypeError("%s every accession column of the DB on one device: this DB is %s.  Run it in one process on one GPU with a "
                        "DB that fits it (SNPMATCH_GPUS unset or one device, no torch.distributed launcher)"
                        % (who_needs, "spread over several GPUs by accession" if isinstance(panel, engine.GroupPanel) or
                           getattr(g, "_shard", None) is not None else "streamed through the device in row slabs"))
    return panel


def _scan_of(g, who_needs, snp_ix):
    """(panel, rows) for a pass-through of ``Genotype`` to a scan of ``engine``: the resident panel, or the refusal that names
    ``who_needs``, and the row filter as ``_rows_or_range`` hands it on.  A function, not a method: the pass-throughs ask of ``g``
    nothing but ``panel()``."""
    return _resident_panel(g, who_needs), _rows_or_range(snp_ix)


def _rows_or_range(snp_ix):
    """a row filter for the panel scans: None (all rows), a ``range`` as it is or where the list is a run ``r, r + 1, ...`` (scanned as
    a dense range), else the list as int64"""
    if snp_ix is None or isinstance(snp_ix, range):
        return snp_ix
    rows = np.asarray(snp_ix, dtype=np.int64).reshape(-1)
    if len(rows) and rows[0] >= 0 and np.array_equal(rows, np.arange(rows[0], rows[0] + len(rows))):
        return range(int(rows[0]), int(rows[0]) + len(rows))
    return rows


def kinship_from_counts(ninfo, same, diff):
    """(same - diff) / ninfo in fp64; 0 / 0 = nan, as ``np.divide`` of the reference's two matrices gives it"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.divide((np.asarray(same, dtype=np.int64) - np.asarray(diff, dtype=np.int64)).astype(np.float64),
                         np.asarray(ninfo).astype(np.float64))


def calc_kinship_mat(snp, return_counts=False):
    """Kinship of a small SNP matrix [n_snp, n_acc] on the host, with the semantics of the reference's function of this name
    (core/snp_genotype.py:440-459): a call >= 0 is informative; 0 counts as -1, 1 as +1, everything else (hets, missing) as 0.
    ``return_counts``: the pair ``(score, informative)`` -- sum of the products (= same - diff) and informative rows per pair of
    accessions, fp64 arrays of exact integers -- else their quotient.  Plain arrays where the reference returns matrices."""
    calls = np.asarray(snp).T                                   # [n_acc, n_snp]
    known = (calls >= 0).astype(np.float64)
    informative = known @ known.T
    signed = np.where(calls == 0, -1.0, np.where(calls == 1, 1.0, 0.0))
    score = signed @ signed.T + 0.0                             # (+ 0.0: a sum of -0.0 products is a plain zero)
    if return_counts:
        return score, informative
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.divide(score, informative)


def af_from_counts(counts, min_informative=0, polarize_geno=1, return_maf=True):
    """Allele frequency from site counts [..., 4] (c0, c1, c2, ninfo): fp64 ``(2 * c[polarize_geno] + c2) / (2 * ninfo)`` -- one
    correctly rounded division of two exact integers --, ``nan`` where ``ninfo <= min_informative``; ``return_maf``: the smaller
    of it and ``1 - it``.  (``polarize_geno=2`` counts a het three times, as the reference's formula does.)"""
    if polarize_geno not in (0, 1, 2):
        raise ValueError("polarize_geno must be 0, 1 or 2, got %r" % (polarize_geno,))
    c = np.asarray(counts).astype(np.int64)
    ninfo = c[..., 3]
    num_alt = 2 * c[..., int(polarize_geno)] + c[..., 2]
    af = np.full(ninfo.shape, np.nan, dtype=np.float64)
    ok = ninfo > min_informative
    with np.errstate(divide="ignore", invalid="ignore"):
        af[ok] = num_alt[ok].astype(np.float64) / (2 * ninfo[ok])
    return np.minimum(af, 1 - af) if return_maf else af


def calculate_af_snp_mat(snp_mat, min_informative=0, polarize_geno=1, return_maf=True):
    """Allele frequency of the rows of a small SNP matrix [n_snp, n_acc] on the host, with the semantics of the reference's function
    of this name (core/snp_genotype.py:360-376): a call other than -1 is informative; returns ``(maf fp64 [n_snp], num_alleles
    int64 [n_snp])``, ``maf`` being ``(2 * #(== polarize_geno) + #(== 2)) / (2 * num_alleles)``, ``nan`` where ``num_alleles <=
    min_informative``, folded to ``min(af, 1 - af)`` with ``return_maf``."""
    calls = np.asarray(snp_mat)
    num_alleles = (calls.shape[1] - np.count_nonzero(calls == -1, axis=1)).astype(np.int64)
    num_alt = 2 * np.count_nonzero(calls == polarize_geno, axis=1).astype(np.int64) + np.count_nonzero(calls == 2, axis=1)
    af = np.full(calls.shape[0], np.nan, dtype=np.float64)
    ok = num_alleles > min_informative
    with np.errstate(divide="ignore", invalid="ignore"):
        af[ok] = num_alt[ok].astype(np.float64) / (2 * num_alleles[ok])
    return (np.minimum(af, 1 - af) if return_maf else af), num_alleles


def _polarize_snps(snps, polarize_geno=1, genotypes=[0, 1]):
    """A copy of a small SNP matrix [n_snp, n_acc] in which the two homozygous codes are exchanged on every row where more than
    half of the columns carry ``polarize_geno`` (core/snp_genotype.py:385-394).  As there, the exchange goes through the value 3:
    a call that already is 3 on such a row comes out as ``genotypes[0]``."""
    assert len(genotypes) == 2, "assuming it is biallelic"
    first, second = genotypes
    out = np.array(snps)
    flip = np.count_nonzero(out == polarize_geno, axis=1) > float(out.shape[1]) / 2
    rows = out[flip]
    out[flip] = np.where(rows == first, second, np.where((rows == second) | (rows == 3), first, rows)).astype(out.dtype)
    return out


def ld_from_counts(counts, v_alt=2, v_het=1, min_n=2):
    """r2 from LD pair counts [..., 9] (n, Ak, Hk, Aj, Hj, AA, AH, HA, HH), the host form of what ``snpm_panel_ld_band`` computes:
    with the genotype values ``v_alt`` for code 1 and ``v_het`` for code 2, int64 ``num = n sxy - sx sy``, ``dx = n sxx - sx^2``,
    ``dy = n syy - sy^2`` and fp64 ``(num * num) / (dx * dy)`` -- three correctly rounded operations on exact integers, the
    device's bits.  ``nan`` where ``n < min_n`` or a row is constant among the common columns."""
    for name, v in (("v_alt", v_alt), ("v_het", v_het)):
        if v not in (0, 1, 2, 3):
            raise ValueError("%s must be 0 .. 3, got %r" % (name, v))
    if min_n < 1:
        raise ValueError("min_n must be at least 1, got %r" % (min_n,))
    c = np.asarray(counts).astype(np.int64)
    va, vh = int(v_alt), int(v_het)
    n = c[..., 0]
    sx, sy = va * c[..., 1] + vh * c[..., 2], va * c[..., 3] + vh * c[..., 4]
    sxx, syy = va * va * c[..., 1] + vh * vh * c[..., 2], va * va * c[..., 3] + vh * vh * c[..., 4]
    sxy = va * va * c[..., 5] + va * vh * (c[..., 6] + c[..., 7]) + vh * vh * c[..., 8]
    num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    r2 = np.full(n.shape, np.nan, dtype=np.float64)
    ok = (n >= min_n) & (dx != 0) & (dy != 0)
    top, bottom = num[ok].astype(np.float64), dx[ok].astype(np.float64) * dy[ok].astype(np.float64)
    r2[ok] = (top * top) / bottom
    return r2


def calculate_ld(snps):
    """Squared Pearson correlation of every pair of rows of a small float matrix [n_snp, n_acc] on the host, with the semantics of
    the reference's function of this name (core/snp_genotype.py:348-358, written there on scipy aliases that scipy has dropped):
    rows are centred and scaled by their population standard deviation, multiplied out and squared.  A ``nan`` in a row, or a
    constant row, makes that row and column ``nan``."""
    x = np.asarray(snps, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
        r = (z @ z.T) / x.shape[1]
    return r * r


def het_from_counts(counts, y_min=5):
    """``c2 / ninfo`` of window counts [..., 4] (c0, c1, c2, ninfo) in fp64: one correctly rounded division, ``nan`` where ``ninfo <=
    y_min`` -- the reference's ``np_get_fraction(.., y_min=5)``"""
    counts = np.asarray(counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        het = counts[..., 2].astype(np.float64) / counts[..., 3].astype(np.float64)
    return np.where(counts[..., 3] <= y_min, np.nan, het)


def mismatch_from_counts(pair_counts):
    """``1.0 - eq / n`` of pair window counts [..., 4] (n, eq, hom_same, hom_diff) in fp64: one division, then one subtraction --
    what ``1 - np.nanmean(..)`` of the reference's 0 / 1 vector does; ``nan`` where ``n == 0``"""
    pair_counts = np.asarray(pair_counts)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = pair_counts[..., 1].astype(np.float64) / pair_counts[..., 0].astype(np.float64)
    return np.where(pair_counts[..., 0] == 0, np.nan, 1.0 - frac)


def _bare_chr_id(name):
    """'Chr1' / 'chr1' / '1' -> '1'"""
    return re.sub("chr", "", str(name), flags=re.IGNORECASE)


class _ChromosomeRows(object):
    """One side of a position intersection: ``order`` = chromosome ids as first named, ``rows[id]`` = its row numbers
    in input order, ``pos`` = all positions as integers."""
    __slots__ = ("order", "rows", "pos")


def _rows_by_chromosome(chrs, pos):
    ins = parsers.ParseInputs("")
    ins.load_snp_info(snpCHR=chrs, snpPOS=pos, snpGT="", snpWEI=np.nan, DPmean=0)
    ins.filter_chr_names()
    side = _ChromosomeRows()
    side.order = [str(c) for c in ins.g_chrs_ids.tolist()]
    side.pos = np.asarray(ins.pos).astype(int)
    side.rows = {}
    if len(side.order):
        names, inv = np.unique(ins.g_chrs, return_inverse=True)
        by_name = np.argsort(inv, kind="stable")                      # rows grouped by chromosome, input order kept
        ends = np.cumsum(np.bincount(inv, minlength=len(names)))
        for k, name in enumerate(names.tolist()):
            side.rows[str(name)] = by_name[(ends[k - 1] if k else 0):ends[k]]
    return side
