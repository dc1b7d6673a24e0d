"""
Thin object layer over the C ABI: Context (one GPU), Panel (DB genotype matrix resident in HBM),
Query (one sample's matched SNPs resident in HBM).  All compute happens in libsnpmatch_hip.so.
"""
import atexit
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import MODE_EXACT, MODE_FAST, MODE_STRICT, check, ptr  # noqa: F401

_default_ctx = None


class Context(object):
    def __init__(self, device_id=0, _borrowed=None):
        lib = _lib.load()
        if _borrowed is None:
            h = C.c_void_p()
            rc = lib.snpm_init(int(device_id), C.byref(h))
            check(rc, None)
        else:                   # a member context of a Group: created and destroyed by the group (snpm_group_create_local)
            h = _borrowed
        self._owns = _borrowed is None
        self.lib = lib
        self.h = h
        self.device_id = int(device_id)
        self._children = weakref.WeakSet()      # panels and queries: freed before the context
        self._pinned = []                       # pinned host blocks handed out by pinned_empty
        self._pinned_bufs = []                  # ... and the ctypes objects their numpy views hang on
        # every context is closed before the interpreter (and with it the HIP runtime) goes down, also when the
        # script ends with an exception; the weak reference keeps the hook from pinning the object.  The library
        # tolerates the other order too (snpm_destroy orphans live panels / queries, include/snpmatch_hip.h).
        ref = weakref.ref(self)
        self._atexit = lambda: (ref() is not None) and ref().close(_at_exit=True)
        atexit.register(self._atexit)

    def close(self, _at_exit=False):
        if self.h:
            kids = list(self._children)
            for k in kids:
                if isinstance(k, Query):
                    k.free()
            for k in kids:
                if isinstance(k, (Panel, Carry, StreamedPanel)):
                    k.free()
            import sys
            if not _at_exit and not sys.is_finalizing():
                # a numpy view of a pinned block that is still referenced would dangle after the free below
                live = [b for b in self._pinned_bufs if sys.getrefcount(b) > 3]
                if live:
                    raise RuntimeError("Context.close(): %d array(s) from pinned_empty() are still referenced; "
                                       "delete them before closing the context" % len(live))
            for blk in self._pinned:
                self.lib.snpm_host_free(self.h, blk)
            self._pinned = []
            self._pinned_bufs = []
            if self._owns:
                self.lib.snpm_destroy(self.h)
            self.h = None
            try:
                atexit.unregister(self._atexit)
            except Exception:
                pass

    def __del__(self):
        try:
            self.close(_at_exit=True)
        except Exception:
            pass

    def set_stream(self, hip_stream):
        """Launch the library's kernels on the given hipStream_t handle (e.g. torch.cuda.Stream().cuda_stream).
        None restores the library's own stream.  Handle 0 (the legacy default stream) is refused: pass a
        real stream so that ordering with the caller's other work is explicit."""
        if hip_stream is None:
            check(self.lib.snpm_set_stream(self.h, None), self.h)
            return
        if int(hip_stream) == 0:
            raise ValueError("set_stream needs a non-default stream handle (got 0); use torch.cuda.Stream()")
        check(self.lib.snpm_set_stream(self.h, C.c_void_p(int(hip_stream))), self.h)

    def synchronize(self):
        check(self.lib.snpm_synchronize(self.h), self.h)

    def row_pitch(self, n_acc, packed=False):
        """bytes per row of a panel of ``n_acc`` accessions on this context (before it is created)"""
        out = C.c_int64(0)
        check(self.lib.snpm_panel_row_pitch(self.h, int(n_acc), 1 if packed else 0, C.byref(out)), self.h)
        return out.value

    def mem_info(self):
        """(free, total) device memory in bytes"""
        f, t = C.c_int64(0), C.c_int64(0)
        check(self.lib.snpm_device_mem_info(self.h, C.byref(f), C.byref(t)), self.h)
        return f.value, t.value

    # ---- profiling (HIP events on the stream the kernels run on)
    def profile(self, on=True):
        check(self.lib.snpm_profile_enable(self.h, 1 if on else 0), self.h)

    def profile_reset(self):
        check(self.lib.snpm_profile_reset(self.h), self.h)

    def profile_read(self, kernel):
        n = C.c_int64(0)
        ms = C.c_double(0)
        check(self.lib.snpm_profile_read(self.h, kernel.encode(), C.byref(n), C.byref(ms)), self.h)
        return n.value, ms.value

    # ---- one-shot forms
    def score_dense(self, wei, db, skip_hets=False):
        """matchGTsAccs on host arrays (fp64 bit-exact with the reference)."""
        db = np.asarray(db)
        wei = np.asarray(wei)
        assert wei.shape[0] == db.shape[0], "please provide same number of positions for both sample and db"
        assert wei.ndim == 2 and wei.shape[1] == 3, "SNP weights should be a np.array with  shape == n,3"
        db = np.ascontiguousarray(db, dtype=np.int8)
        wei = np.ascontiguousarray(wei, dtype=np.float64)
        n, n_acc = db.shape
        score = np.zeros(n_acc, dtype=np.float64)
        ninfo = np.zeros(n_acc, dtype=np.int64)
        if n_acc == 0:
            return score, ninfo
        check(self.lib.snpm_score_dense_host(self.h, ptr(db), n_acc, n, n_acc, ptr(wei), int(bool(skip_hets)),
                                             ptr(score), ptr(ninfo)), self.h)
        return score, ninfo

    def likelihood_device(self, d_y, d_n, m, length, d_lik, d_lrt, truncate=False, amin=None, check_domain=False):
        """likeliTest rows on device pointers (no host round trip unless check_domain)."""
        a = float("nan") if amin is None else float(amin)
        dom = C.c_int(0)
        check(self.lib.snpm_likelihood_device(self.h, C.c_void_p(d_y), C.c_void_p(d_n), int(m), int(length),
                                              int(bool(truncate)), a, C.c_void_p(d_lik), C.c_void_p(d_lrt),
                                              C.byref(dom) if check_domain else None), self.h)
        if check_domain and dom.value:
            raise AssertionError("provided y is greater than n")

    def likelihood(self, y, n, truncate=False, amin=None):
        """Rows of (matches y, informative n) -> (likelihood, ratio to the row minimum)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        assert y.shape == n.shape
        shape = y.shape
        if y.ndim == 1:
            m, ln = 1, y.shape[0]
        else:
            m, ln = y.shape
        lik = np.empty(shape, dtype=np.float64)
        lrt = np.empty(shape, dtype=np.float64)
        if y.size == 0:
            return lik, lrt
        a = float("nan") if amin is None else float(amin)
        check(self.lib.snpm_likelihood(self.h, ptr(y), ptr(n), m, ln, int(bool(truncate)), a, ptr(lik), ptr(lrt)), self.h)
        return lik, lrt

    def sample_synthetic(self, seed, snp0, n, planted, d_wei, err=0.02, frac_pl=0.8):
        """Benchmark sample generated on the device into ``d_wei`` (raw device pointer of a float64 [n, 3] buffer):
        accession ``planted`` of the synthetic panel ``seed`` with a fraction ``err`` of random calls and a fraction
        ``frac_pl`` of PL-derived weights.  ``snpmatch_amd.synth.sample_weights_twin`` is the numpy twin."""
        from . import synth
        tab = synth.exp_table()
        check(self.lib.snpm_sample_synthetic(self.h, C.c_uint64(int(seed)), int(snp0), int(n), int(planted),
                                             int(round(err * 1000)), int(round(frac_pl * 1000)), ptr(tab),
                                             C.c_void_p(int(d_wei))), self.h)

    def pinned_empty(self, shape, dtype):
        """numpy array in pinned host memory (hipHostMalloc): inputs of ``score_batch`` built here skip the staging copy.
        The block is released when the context closes: the array (and every view of it) must not be used after
        ``close()`` -- ``close`` refuses while such arrays are still referenced elsewhere."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        h = C.c_void_p()
        check(self.lib.snpm_host_alloc(self.h, n, C.byref(h)), self.h)
        buf = (C.c_char * max(n, 1)).from_address(h.value)
        self._pinned.append(h)
        self._pinned_bufs.append(buf)           # numpy arrays made from it hold references to this ctypes object
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def binom_identity(self, x, n, error_rate=0.0005, pthres=0.05, return_sf=False):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        out = np.empty(len(x), dtype=np.int64)
        sf = np.empty(len(x), dtype=np.float64)
        check(self.lib.snpm_binom_identity(self.h, ptr(x), ptr(n), len(x), float(error_rate), float(pthres), ptr(out),
                                           ptr(sf)), self.h)
        return (out, sf) if return_sf else out


def default_context():
    """Process-wide context on the device named by SNPMATCH_DEVICE / LOCAL_RANK (default 0)."""
    global _default_ctx
    if _default_ctx is None:
        import os
        dev = int(os.environ.get("SNPMATCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _default_ctx = Context(dev)         # closed at interpreter exit by its own atexit hook
    return _default_ctx


class RowStore(object):
    """Where the rows of a DB come from on the host side: a flat file of int8 rows (``npy=``: a C-ordered int8 .npy, read
    natively with pread / O_DIRECT by the library) or an array-like ``snps`` [n_snp, n_acc] (numpy array, memmap, h5py
    dataset: sliced here, uploaded from host memory).  ``load`` puts rows into a panel through the pinned staging path --
    the counterpart of the reference's ``g.g.snps[idx, :]`` (core/snpmatch.py:222, pygwas/genotype.py:548-550)."""

    def __init__(self, snps=None, npy=None, h5=None, npy_packed=None):
        assert (snps is not None) + (npy is not None) + (h5 is not None) + (npy_packed is not None) == 1
        self.snps, self.path, self.offset, self.h5, self.packed_file = snps, None, 0, h5, False
        if npy_packed is not None:          # (path of a uint8 .npy [n_snp, ceil(n_acc / 4)] with 2 bits per call, n_acc): a packed .snpm
            npy, n_acc_true = npy_packed
            with open(npy, "rb") as fh:
                major, _ = np.lib.format.read_magic(fh)
                shape, fortran, dtype = (np.lib.format.read_array_header_1_0(fh) if major == 1
                                         else np.lib.format.read_array_header_2_0(fh))
                self.offset = fh.tell()
            assert len(shape) == 2 and not fortran and np.dtype(dtype) == np.uint8 and shape[1] == (int(n_acc_true) + 3) // 4, \
                "expected a C-ordered uint8 matrix of 2-bit calls"
            self.path, self.n_snp, self.n_acc, self.packed_file, self.file_pitch = npy, int(shape[0]), int(n_acc_true), True, int(shape[1])
        elif h5 is not None:                  # (snpmatch_amd.h5.File, dataset name): the reference's HDF5 DB, read natively
            ds = h5[0][h5[1]]
            assert ds.ndim == 2 and ds.dtype == np.int8, "expected a 2-D int8 dataset"
            self.n_snp, self.n_acc = int(ds.shape[0]), int(ds.shape[1])
        elif npy is not None:
            with open(npy, "rb") as fh:
                major, _ = np.lib.format.read_magic(fh)
                shape, fortran, dtype = (np.lib.format.read_array_header_1_0(fh) if major == 1
                                         else np.lib.format.read_array_header_2_0(fh))
                self.offset = fh.tell()
            assert len(shape) == 2 and not fortran and np.dtype(dtype) == np.int8, "expected a C-ordered int8 matrix"
            self.path, self.n_snp, self.n_acc = npy, int(shape[0]), int(shape[1])
        else:
            self.n_snp, self.n_acc = int(snps.shape[0]), int(snps.shape[1])

    def load(self, panel, cols, rows, row0, nrows=None, slab_rows=1 << 16):
        """panel rows [row0, row0 + n) <- DB rows ``rows`` (an increasing int64 list; None: the range [0, nrows), or
        (first, n) for a range), columns cols = (a0, a1)"""
        a0, a1 = cols
        assert a1 - a0 == panel.n_acc
        if rows is None:
            rows = (0, self.n_snp if nrows is None else nrows)
        if not isinstance(rows, tuple):
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            if len(rows) and int(rows[-1]) - int(rows[0]) + 1 == len(rows) and (len(rows) < 2 or bool(np.all(np.diff(rows) == 1))):
                rows = (int(rows[0]), len(rows))            # a contiguous run: the range form (one big read per thread)
        if self.h5 is not None:
            if isinstance(rows, tuple):
                panel.load_h5(self.h5[0], self.h5[1], a0, None, rows[0], row0, rows[1])
            else:
                panel.load_h5(self.h5[0], self.h5[1], a0, rows, 0, row0, len(rows))
            return
        if self.packed_file:
            assert a0 % 4 == 0, "accession shards of a packed DB start at multiples of 4"
            if isinstance(rows, tuple):
                panel.load_file_rows_packed(self.path, self.offset, self.file_pitch, a0, None, rows[0], row0, rows[1])
            else:
                panel.load_file_rows_packed(self.path, self.offset, self.file_pitch, a0, rows, 0, row0, len(rows))
            return
        if self.path is not None:
            if isinstance(rows, tuple):
                panel.load_file_rows(self.path, self.offset, self.n_acc, a0, None, rows[0], row0, rows[1])
            else:
                panel.load_file_rows(self.path, self.offset, self.n_acc, a0, rows, 0, row0, len(rows))
            return
        whole = (a0 == 0 and a1 == self.n_acc)
        if isinstance(rows, tuple):
            for r in range(rows[0], rows[0] + rows[1], slab_rows):
                r1 = min(r + slab_rows, rows[0] + rows[1])
                blk = self.snps[r:r1] if whole else self.snps[r:r1, a0:a1]
                panel.upload_rows(row0 + r - rows[0], np.ascontiguousarray(blk, dtype=np.int8))
        else:
            for i in range(0, len(rows), slab_rows):
                idx = rows[i:i + slab_rows]
                blk = self.snps[idx, :] if whole else self.snps[idx, a0:a1]      # the reference's fancy row read
                panel.upload_rows(row0 + i, np.ascontiguousarray(blk, dtype=np.int8))


_default_group = None


def device_count():
    n = C.c_int(0)
    check(_lib.load().snpm_device_count(C.byref(n)), None)
    return n.value


def group_devices():
    """Device ids of the GPUs one process should drive, or None for a single GPU.  SNPMATCH_GPUS = "all" (default when
    several GPUs are visible and no torch.distributed job is active), a count, or a comma-separated list of device ids
    (a device named twice needs SNPMATCH_GROUP_LOOPBACK=1: rehearsal of the sharded path on a one-GPU box)."""
    import os
    spec = os.environ.get("SNPMATCH_GPUS", "all").strip().lower()
    if "," in spec:
        ids = [int(x) for x in spec.split(",") if x.strip() != ""]
    else:
        n_vis = device_count()
        n = n_vis if spec in ("", "all") else max(1, min(int(spec), n_vis))
        first = int(os.environ.get("SNPMATCH_DEVICE", "0"))
        ids = [(first + i) % max(n_vis, 1) for i in range(n)]
    return ids if len(ids) > 1 else None


def default_group(n_members=None):
    """Process-wide ``Group`` over ``group_devices()`` (first ``n_members`` of them), created on first use; None for one GPU."""
    global _default_group
    import os
    ids = group_devices()
    if ids is None:
        return None
    if n_members is not None:
        ids = ids[:max(1, int(n_members))]
        if len(ids) < 2:
            return None
    if _default_group is not None and _default_group.h and [c.device_id for c in _default_group.contexts] == ids:
        return _default_group
    if _default_group is not None:
        _default_group.free()
    loopback = os.environ.get("SNPMATCH_GROUP_LOOPBACK", "0") not in ("", "0")
    _default_group = Group.local(ids, loopback=loopback)
    return _default_group


class Panel(object):
    """int8 [n_snp, n_acc] genotype matrix in HBM (SNP-major, row pitch padded to 256 B; to 128 B where that saves 5 % of the row)."""

    def __init__(self, ctx, n_snp, n_acc, packed=False, n_acc_total=None):
        self.ctx = ctx
        self.n_snp = int(n_snp)
        self.n_acc = int(n_acc)
        self.packed = bool(packed)      # 2 bits per call instead of one byte (same results, 4x less HBM)
        h = C.c_void_p()
        create = ctx.lib.snpm_panel_create_packed if packed else ctx.lib.snpm_panel_create
        check(create(ctx.h, self.n_snp, self.n_acc, C.byref(h)), ctx.h)
        self.h = h
        if n_acc_total is not None and int(n_acc_total) != self.n_acc:
            # a shard of a wider DB: the reference-order kernels follow the summation rule of the WHOLE panel's width
            # (numpy sums a one-accession panel pairwise, core/snpmatch.py:85-87; every wider one row after row)
            check(ctx.lib.snpm_panel_set_total_accessions(h, int(n_acc_total)), ctx.h)
        pitch = C.c_int64(0)
        dptr = C.c_void_p()
        check(ctx.lib.snpm_panel_info(h, None, None, C.byref(pitch), C.byref(dptr)), ctx.h)
        self.pitch = pitch.value
        self.device_ptr = dptr.value
        self._queries = weakref.WeakSet()
        ctx._children.add(self)

    @classmethod
    def from_host(cls, ctx, snps, slab_rows=1 << 16, packed=False, cols=None):
        """Upload an array-like [n_snp, n_acc] (numpy array, memmap or h5py dataset) slab by slab; ``cols`` = (a0, a1)
        keeps only that accession range (this rank's shard of an accession-sharded job)."""
        return cls.from_store(ctx, RowStore(snps=snps), packed=packed, cols=cols)

    @classmethod
    def from_store(cls, ctx, store, packed=False, cols=None):
        """the whole DB (or its columns ``cols``) resident: every row through the staging path"""
        a0, a1 = (0, store.n_acc) if cols is None else cols
        p = cls(ctx, store.n_snp, a1 - a0, packed=packed, n_acc_total=store.n_acc)
        try:
            store.load(p, (a0, a1), None, 0, store.n_snp)
        except Exception:
            p.free()
            raise
        return p            # returns once the last slab is enqueued; scoring calls wait for the copies on the device

    def query(self, row_idx, wei, row0=0):
        """the matched SNPs of one sample against this panel (``GroupPanel`` / ``StreamedPanel`` offer the same call)"""
        return Query(self, row_idx, wei, row0=row0)

    def genotype_once(self, row_idx, wei, sample_idx=None, chunk=1000, skip_hets=False, mode=MODE_EXACT, likelihoods=True, table=None):
        """ONE sample in ONE call (snpm_genotype_once): ``row_idx`` int64 [n] matched DB rows, ``wei`` float64 [n_wei, 3] the
        sample's weights, ``sample_idx`` int64 [n] the weight row of each matched SNP (None: rows 0..n-1).  With ``table``
        (float64 [<= 65536]) ``wei`` holds uint16 codes instead, weight = table[code] (snpm_genotype_once_coded: 10 instead of 32
        bytes per matched SNP over PCIe).  Returns a dict with score / ninfo (and lik / lrt of the truncated counts) [n_acc] and
        the re-evaluation counters of ``Query.run``."""
        ctx = self.ctx
        row_idx = np.ascontiguousarray(row_idx, dtype=np.int64)
        wei = np.asarray(wei)
        assert wei.ndim == 2 and wei.shape[1] == 3, "SNP weights should be a np.array with  shape == n,3"
        wei = np.ascontiguousarray(wei, dtype=np.float64 if table is None else np.uint16)
        if sample_idx is not None:
            sample_idx = np.ascontiguousarray(sample_idx, dtype=np.int64)
            assert len(sample_idx) == len(row_idx), "please provide same number of positions for both sample and db"
        else:
            assert len(wei) == len(row_idx), "please provide same number of positions for both sample and db"
        out = {"score": np.empty(self.n_acc, dtype=np.float64), "ninfo": np.empty(self.n_acc, dtype=np.int64)}
        if likelihoods:
            out["lik"] = np.empty(self.n_acc, dtype=np.float64)
            out["lrt"] = np.empty(self.n_acc, dtype=np.float64)
        info = np.zeros(4, dtype=np.int64)
        if table is not None:
            table = np.ascontiguousarray(table, dtype=np.float64)
            assert table.ndim == 1 and 1 <= len(table) <= 65536
            check(ctx.lib.snpm_genotype_once_coded(self.h, ptr(row_idx), ptr(wei), ptr(table), len(table), ptr(sample_idx), len(wei),
                                                   len(row_idx), int(chunk), int(bool(skip_hets)), int(mode), ptr(out["score"]),
                                                   ptr(out["ninfo"]), ptr(out.get("lik")), ptr(out.get("lrt")), ptr(info)), ctx.h)
        else:
            check(ctx.lib.snpm_genotype_once(self.h, ptr(row_idx), ptr(wei), ptr(sample_idx), len(wei), len(row_idx), int(chunk),
                                             int(bool(skip_hets)), int(mode), ptr(out["score"]), ptr(out["ninfo"]), ptr(out.get("lik")),
                                             ptr(out.get("lrt")), ptr(info)), ctx.h)
        out["n_strict_reeval"], out["all_integer_weights"], out["reeval_path"] = int(info[0]), bool(info[1]), int(info[2])
        return out

    def upload_rows(self, row0, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int8)
        assert rows.ndim == 2 and rows.shape[1] == self.n_acc
        check(self.ctx.lib.snpm_panel_upload_rows(self.h, int(row0), rows.shape[0], ptr(rows), rows.shape[1]), self.ctx.h)

    def load_file(self, path, file_offset, row0=0, nrows=None):
        """Stream rows from a file of tightly packed int8 rows (native flat panel) through the staging path."""
        nrows = self.n_snp - row0 if nrows is None else nrows
        check(self.ctx.lib.snpm_panel_load_file(self.h, str(path).encode(), int(file_offset), int(row0), int(nrows)), self.ctx.h)

    def load_file_rows(self, path, file_offset, file_pitch, col0=0, row_idx=None, file_row0=0, row0=0, nrows=None):
        """rows from a file holding an int8 matrix of ``file_pitch`` bytes per row: file rows ``row_idx`` (or file_row0 ..),
        columns [col0, col0 + n_acc) -> panel rows [row0, row0 + nrows)  (snpm_panel_load_file_rows)"""
        if row_idx is not None:
            row_idx = np.ascontiguousarray(row_idx, dtype=np.int64)
            nrows = len(row_idx) if nrows is None else nrows
        check(self.ctx.lib.snpm_panel_load_file_rows(self.h, str(path).encode(), int(file_offset), int(file_pitch), int(col0),
                                                     ptr(row_idx), int(file_row0), int(row0), int(nrows)), self.ctx.h)

    def load_file_rows_packed(self, path, file_offset, file_pitch, acc0=0, row_idx=None, file_row0=0, row0=0, nrows=None):
        """rows from a PACKED flat file (2 bits per call, ``file_pitch`` bytes per row): accessions [acc0, acc0 + n_acc), acc0 % 4 == 0"""
        if row_idx is not None:
            row_idx = np.ascontiguousarray(row_idx, dtype=np.int64)
            nrows = len(row_idx) if nrows is None else nrows
        check(self.ctx.lib.snpm_panel_load_file_rows_packed(self.h, str(path).encode(), int(file_offset), int(file_pitch), int(acc0),
                                                            ptr(row_idx), int(file_row0), int(row0), int(nrows)), self.ctx.h)

    def load_h5(self, h5_file, dataset, col0=0, row_idx=None, file_row0=0, row0=0, nrows=None):
        """rows of a 2-D int8 dataset of an open ``snpmatch_amd.h5.File`` (the reference's DB format): the loader's threads read
        and decompress the chunks straight into the staging slabs (snpm_panel_load_h5)"""
        if row_idx is not None:
            row_idx = np.ascontiguousarray(row_idx, dtype=np.int64)
            nrows = len(row_idx) if nrows is None else nrows
        check(self.ctx.lib.snpm_panel_load_h5(self.h, h5_file.h, dataset.encode(), int(col0), ptr(row_idx), int(file_row0), int(row0),
                                              int(nrows)), self.ctx.h)

    @classmethod
    def from_npy(cls, ctx, path, packed=False, cols=None):
        """Panel from an int8 [n_snp, n_acc] .npy file (C order), read natively (no numpy copy)."""
        return cls.from_store(ctx, RowStore(npy=path), packed=packed, cols=cols)

    def upload_wait(self):
        check(self.ctx.lib.snpm_panel_upload_wait(self.h), self.ctx.h)

    def download_rows(self, row0, nrows):
        out = np.empty((int(nrows), self.n_acc), dtype=np.int8)
        check(self.ctx.lib.snpm_panel_download_rows(self.h, int(row0), int(nrows), ptr(out), self.n_acc), self.ctx.h)
        return out

    def fill_synthetic(self, seed, snp0=0, acc0=0, row0=0, nrows=None):
        """rows [row0, row0 + nrows) <- SNPs snp0 .. of the synthetic panel ``seed`` (columns acc0 ..)"""
        nrows = self.n_snp - row0 if nrows is None else nrows
        check(self.ctx.lib.snpm_panel_fill_synthetic_rows(self.h, C.c_uint64(int(seed)), int(snp0), int(acc0), int(row0),
                                                          int(nrows)), self.ctx.h)

    def segregating_rows(self, cols):
        """uint8 mask [n_snp]: 1 where the informative calls of accessions `cols` differ (device scan)."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        mask = np.zeros(self.n_snp, dtype=np.uint8)
        check(self.ctx.lib.snpm_panel_segregating(self.h, ptr(cols), len(cols), ptr(mask)), self.ctx.h)
        return mask

    def segregating_first(self, cols):
        """(mask, first) for an accession-sharded DB: local mask and the first informative call per row (0xFF: none)"""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        mask = np.zeros(self.n_snp, dtype=np.uint8)
        first = np.full(self.n_snp, 0xFF, dtype=np.uint8)
        check(self.ctx.lib.snpm_panel_segregating_first(self.h, ptr(cols), len(cols), ptr(mask), ptr(first)), self.ctx.h)
        return mask, first

    def stream_read(self):
        """PMC calibration: read every panel byte once; returns the byte count."""
        n = C.c_int64(0)
        check(self.ctx.lib.snpm_debug_stream_read(self.h, C.byref(n)), self.ctx.h)
        return n.value

    def free(self):
        if self.h:
            for q in list(self._queries):
                q.free()
            if self.ctx.h:
                self.ctx.lib.snpm_panel_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Query(object):
    """A sample's matched SNPs (panel rows + weights) resident on the device."""

    def __init__(self, panel, row_idx, wei, row0=0, _device=None):
        self.panel = panel
        ctx = panel.ctx
        if _device is not None:             # (d_row_idx or None, d_wei, n): raw device pointers, see from_device
            d_rows, d_wei, n = _device
            self.n = int(n)
            h = C.c_void_p()
            check(ctx.lib.snpm_query_create_device(panel.h, C.c_void_p(d_rows) if d_rows else None, int(row0), self.n,
                                                   C.c_void_p(int(d_wei)), C.byref(h)), ctx.h)
            self.h = h
            panel._queries.add(self)
            ctx._children.add(self)
            return
        wei = np.asarray(wei)
        assert wei.ndim == 2 and wei.shape[1] == 3, "SNP weights should be a np.array with  shape == n,3"
        wei = np.ascontiguousarray(wei, dtype=np.float64)
        n = wei.shape[0]
        if row_idx is not None:
            row_idx = np.ascontiguousarray(row_idx, dtype=np.int64)
            assert row_idx.shape == (n,), "please provide same number of positions for both sample and db"
        self.n = n
        h = C.c_void_p()
        check(ctx.lib.snpm_query_create(panel.h, ptr(row_idx), int(row0), n, ptr(wei), C.byref(h)), ctx.h)
        self.h = h
        panel._queries.add(self)
        ctx._children.add(self)

    @classmethod
    def from_device(cls, panel, d_row_idx, d_wei, n, row0=0):
        """Query whose row list (int64 [n] or None = dense from ``row0``) and weights (float64 [n, 3]) already are
        in device memory (raw pointers); they are copied."""
        return cls(panel, None, None, row0=row0, _device=(d_row_idx, d_wei, n))

    def run(self, chunk=1000, skip_hets=False, mode=MODE_EXACT, return_info=False):
        """Genotyper.genotyper accumulators: (ScoreList float64 [n_acc], NumInfoSites int64 [n_acc])."""
        ctx = self.panel.ctx
        score = np.empty(self.panel.n_acc, dtype=np.float64)
        ninfo = np.empty(self.panel.n_acc, dtype=np.int64)
        info = np.zeros(4, dtype=np.int64) if return_info else None
        check(ctx.lib.snpm_query_run(self.h, int(chunk), int(bool(skip_hets)), int(mode), ptr(score), ptr(ninfo), ptr(info)),
              ctx.h)
        if return_info:
            return score, ninfo, {"n_strict_reeval": int(info[0]), "all_integer_weights": bool(info[1]),
                                  "reeval_path": int(info[2])}
        return score, ninfo

    def run_device(self, chunk=1000, skip_hets=False, mode=MODE_EXACT):
        """Enqueue the scoring (nothing waits on the host, the certificate included); returns raw device pointers
        (d_score f64[n_acc], d_ninfo i64[n_acc]).  ``last_reeval()`` reads the re-evaluation count afterwards."""
        ctx = self.panel.ctx
        ds, dn = C.c_void_p(), C.c_void_p()
        check(ctx.lib.snpm_query_run_device(self.h, int(chunk), int(bool(skip_hets)), int(mode), C.byref(ds), C.byref(dn),
                                            None), ctx.h)
        return ds.value, dn.value

    def last_reeval(self):
        """accessions the last certified run re-evaluated in reference order (synchronises)"""
        n = C.c_int64(0)
        check(self.panel.ctx.lib.snpm_query_last_reeval(self.h, C.byref(n)), self.panel.ctx.h)
        return n.value

    def last_kernel(self):
        return (self.panel.ctx.lib.snpm_query_last_kernel(self.h) or b"").decode()

    def run_carry(self, carry, chunk=1000, skip_hets=False, mode=MODE_EXACT, chunks_after=0):
        """score these rows as the next SNP slab of a larger job (see ``Carry`` / ``SlabScorer``)"""
        ctx = self.panel.ctx
        check(ctx.lib.snpm_query_run_carry(self.h, int(chunk), int(bool(skip_hets)), int(mode), int(chunks_after), carry.h),
              ctx.h)

    def bind_outputs(self, d_score, d_ninfo):
        """Write results of later runs into caller-owned device buffers (raw pointers, e.g. tensor.data_ptr())."""
        ctx = self.panel.ctx
        check(ctx.lib.snpm_query_bind_outputs(self.h, C.c_void_p(d_score) if d_score else None,
                                              C.c_void_p(d_ninfo) if d_ninfo else None), ctx.h)

    def error_bound(self, chunk=1000):
        b = C.c_double(0)
        check(self.panel.ctx.lib.snpm_query_error_bound(self.h, int(chunk), C.byref(b)), self.panel.ctx.h)
        return b.value

    def run_windows(self, win_off, skip_hets=False, totals=True, fast=False):
        """Per-window matchGTsAccs: (score [n_win,n_acc], ninfo [n_win,n_acc], tot_score, tot_ninfo).
        ``fast``: the segmented streaming pass with the certificate (exact counts, scores to ~1e-12) instead of the
        reference-order pass (fp64 bits); ``self.last_windows_info`` then holds the re-evaluation counters."""
        ctx = self.panel.ctx
        if fast:
            win_off = np.ascontiguousarray(win_off, dtype=np.int64)
            n_win = len(win_off) - 1
            na = self.panel.n_acc
            score = np.empty((n_win, na), dtype=np.float64)
            ninfo = np.empty((n_win, na), dtype=np.int64)
            ts = np.empty(na, dtype=np.float64)
            tn = np.empty(na, dtype=np.int64)
            info = np.zeros(4, dtype=np.int64)
            check(ctx.lib.snpm_query_run_windows_fast(self.h, ptr(win_off), n_win, int(bool(skip_hets)), ptr(score), ptr(ninfo),
                                                      ptr(ts), ptr(tn), ptr(info)), ctx.h)
            self.last_windows_info = {"pairs_reeval": int(info[0]), "totals_reeval": int(info[1]), "strict_fallback": bool(info[2])}
            return score, ninfo, ts, tn
        win_off = np.ascontiguousarray(win_off, dtype=np.int64)
        n_win = len(win_off) - 1
        na = self.panel.n_acc
        score = np.empty((n_win, na), dtype=np.float64)
        ninfo = np.empty((n_win, na), dtype=np.int64)
        ts = np.empty(na, dtype=np.float64)
        tn = np.empty(na, dtype=np.int64)
        check(ctx.lib.snpm_query_run_windows(self.h, ptr(win_off), n_win, int(bool(skip_hets)), ptr(score), ptr(ninfo),
                                             ptr(ts) if totals else None, ptr(tn) if totals else None), ctx.h)
        return score, ninfo, ts, tn

    def gather_columns(self, acc_idx):
        """calls of accessions ``acc_idx`` at the matched rows: uint8 [len(acc_idx), n] (0xFF = missing)"""
        acc_idx = np.ascontiguousarray(acc_idx, dtype=np.int32)
        out = np.full((len(acc_idx), self.n), 0xFF, dtype=np.uint8)
        check(self.panel.ctx.lib.snpm_query_gather_columns(self.h, ptr(acc_idx), len(acc_idx), ptr(out)), self.panel.ctx.h)
        return out

    def f1_pairs(self, acc_idx):
        """In-silico crosses of every pair of ``acc_idx`` (order of itertools.combinations) over the query's
        rows: (score float64 [n_pairs] with numpy's np.sum bits, ninfo int64 [n_pairs])."""
        ctx = self.panel.ctx
        acc_idx = np.ascontiguousarray(acc_idx, dtype=np.int32)
        k = len(acc_idx)
        n_pairs = k * (k - 1) // 2
        score = np.zeros(n_pairs, dtype=np.float64)
        ninfo = np.zeros(n_pairs, dtype=np.int64)
        check(ctx.lib.snpm_query_f1_pairs(self.h, ptr(acc_idx), k, ptr(score), ptr(ninfo)), ctx.h)
        return score, ninfo

    def free(self):
        if self.h:
            if self.panel.ctx.h and self.panel.h:
                self.panel.ctx.lib.snpm_query_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def cross_calls(ctx, codes, p1, p2, win_off, lr_thres, n_marker_thres=5, return_counts=False):
    """genotype_cross in one device call (``snpm_cross_calls``): ``codes`` uint8 [n, n_samples] call codes of the F2 samples at
    the matched segregating markers (rows in window order; a row-strided view such as ``m[:, :k]`` is passed as it is), ``p1`` /
    ``p2`` the parents' calls (0 / 1 / 2, different), ``win_off`` [n_win + 1] the markers of every window.  Returns ``geno`` int8
    [n_win, n_samples] (-1 NA, 0 parent 1, 1 heterozygous, 2 parent 2) and, with ``return_counts``, also int32 [n_win, n_samples,
    3] = (m1, mh, m2).  ``ctx`` None: the library only validates (a sound call then fails for want of a context)."""
    codes = np.asarray(codes)
    assert codes.ndim == 2 and codes.dtype == np.uint8, "codes: uint8 [n, n_samples]"
    n, ns = codes.shape
    if n > 1 and ns > 0 and codes.strides[1] == 1 and codes.strides[0] >= ns:
        ld = codes.strides[0]               # rows with padding behind them travel as they are
    else:
        codes, ld = np.ascontiguousarray(codes), ns
    p1 = np.ascontiguousarray(p1, dtype=np.int8)
    p2 = np.ascontiguousarray(p2, dtype=np.int8)
    assert len(p1) == n and len(p2) == n, "one parental call per marker"
    win_off = np.ascontiguousarray(win_off, dtype=np.int64)
    n_win = len(win_off) - 1
    assert n_win >= 0, "win_off holds n_win + 1 entries"
    geno = np.empty((n_win, ns), dtype=np.int8)
    counts = np.empty((n_win, ns, 3), dtype=np.int32) if return_counts else None
    lib = ctx.lib if ctx is not None else _lib.load()
    h = ctx.h if ctx is not None else None
    check(lib.snpm_cross_calls(h, ptr(codes), n, ns, ld, ptr(p1), ptr(p2), ptr(win_off), n_win, float(lr_thres), int(n_marker_thres),
                               ptr(geno), ptr(counts)), h)
    return (geno, counts) if return_counts else geno


def cross_hmm(ctx, codes, depth_rank, pair, chain_off, logT, logI, logE, return_omega=False):
    """genotype_cross_hmm in one device call (``snpm_cross_hmm``): the 3-state Viterbi path of every (chain, sample).  ``codes``
    uint8 and ``depth_rank`` uint16, both [n, n_samples] (markers chain by chain; row-strided views with one common stride
    travel as they are), ``pair`` [n] the ordered parental pair 0..5, ``chain_off`` [n_chain + 1], ``logT`` [n_chain, 3, 3],
    ``logI`` / ``logE`` [6, n_depth, 4, 3] (``core.infer`` builds them with numpy).  Returns ``state`` int8 [n, n_samples] and, with
    ``return_omega``, also float64 [n, n_samples, 3].  ``ctx`` None: the library only validates."""
    codes, depth_rank = np.asarray(codes), np.asarray(depth_rank)
    assert codes.ndim == 2 and codes.dtype == np.uint8, "codes: uint8 [n, n_samples]"
    assert depth_rank.shape == codes.shape and depth_rank.dtype == np.uint16, "depth_rank: uint16 of the shape of codes"
    n, ns = codes.shape
    if (n > 1 and ns > 0 and codes.strides[1] == 1 and depth_rank.strides[1] == 2 and codes.strides[0] >= ns
            and depth_rank.strides[0] == 2 * codes.strides[0]):
        ld = codes.strides[0]               # rows with padding behind them travel as they are
    else:
        codes, depth_rank, ld = np.ascontiguousarray(codes), np.ascontiguousarray(depth_rank), ns
    pair = np.ascontiguousarray(pair, dtype=np.uint8)
    assert len(pair) == n, "one parental pair per marker"
    chain_off = np.ascontiguousarray(chain_off, dtype=np.int64)
    n_chain = len(chain_off) - 1
    assert n_chain >= 0, "chain_off holds n_chain + 1 entries"
    logT = np.ascontiguousarray(logT, dtype=np.float64)
    logI = np.ascontiguousarray(logI, dtype=np.float64)
    logE = np.ascontiguousarray(logE, dtype=np.float64)
    assert logT.shape == (n_chain, 3, 3), "logT: [n_chain, 3, 3]"
    assert logI.ndim == 4 and logI.shape[0] == 6 and logI.shape[2:] == (4, 3) and logE.shape == logI.shape, "logI / logE: [6, n_depth, 4, 3]"
    n_depth = logI.shape[1]
    state = np.empty((n, ns), dtype=np.int8)
    omega = np.empty((n, ns, 3), dtype=np.float64) if return_omega else None
    lib = ctx.lib if ctx is not None else _lib.load()
    h = ctx.h if ctx is not None else None
    check(lib.snpm_cross_hmm(h, ptr(codes), ptr(depth_rank), n, ns, ld, ptr(pair), ptr(chain_off), n_chain, ptr(logT), ptr(logI),
                             ptr(logE), n_depth, ptr(state), ptr(omega)), h)
    return (state, omega) if return_omega else state


PAIR_MAX_ID = 127          # ids of ``pair_counts``: the high bit of every byte is free for the kernel's byte-parallel tests


def pair_counts(ctx, ids, seg_off):
    """pairsnp for every pair of a set of samples in one device call (``snpm_pair_counts``): ``ids`` uint8 [n, n_samples], 0 = the
    sample has no call at the record, 1..127 = the id of its genotype text (a row-strided view such as ``m[:, :k]`` is passed as it
    is), ``seg_off`` [n_seg + 1] the records of every segment (chromosome).  Returns ``(common, match)``, both int32 [n_seg,
    n_samples, n_samples]: records both samples have a call at, and records at which the two calls are the same text.  ``ctx``
    None: the library only validates (a sound call then fails for want of a context)."""
    ids = np.asarray(ids)
    assert ids.ndim == 2 and ids.dtype == np.uint8, "ids: uint8 [n, n_samples]"
    n, ns = ids.shape
    if n > 1 and ns > 0 and ids.strides[1] == 1 and ids.strides[0] >= ns:
        ld = ids.strides[0]                 # rows with padding behind them travel as they are
    else:
        ids, ld = np.ascontiguousarray(ids), ns
    seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
    n_seg = len(seg_off) - 1
    assert n_seg >= 0, "seg_off holds n_seg + 1 entries"
    lib = ctx.lib if ctx is not None else _lib.load()
    h = ctx.h if ctx is not None else None
    if n_seg * ns * ns > (1 << 27):         # the library's limit, before numpy is asked for the result arrays
        check(lib.snpm_pair_counts(h, ptr(ids), n, ns, ld, ptr(seg_off), n_seg, None, None), h)
    common = np.empty((n_seg, ns, ns), dtype=np.int32)
    match = np.empty((n_seg, ns, ns), dtype=np.int32)
    check(lib.snpm_pair_counts(h, ptr(ids), n, ns, ld, ptr(seg_off), n_seg, ptr(common), ptr(match)), h)
    return common, match


def _need_resident_panel(panel, caller):
    """the refusal of ``kinship_counts`` / ``site_counts`` for group (accession-sharded) and streamed panels"""
    if not isinstance(panel, Panel):
        raise TypeError("%s needs every accession column on one device: a %s is %s, load the DB as one resident "
                        "panel (int8 or packed) on one GPU" % (caller, type(panel).__name__, "spread over several GPUs by accession"
                                                               if isinstance(panel, GroupPanel) else "not a resident panel"))


def _row_selection(panel, rows):
    """``rows`` (None, a ``slice`` / ``range`` of step 1, or an index array) as the library's ``(row_idx, row0, n_rows)``"""
    if rows is None:
        return None, 0, panel.n_snp
    if isinstance(rows, (slice, range)):
        r = range(*rows.indices(panel.n_snp)) if isinstance(rows, slice) else rows
        if r.step != 1:
            raise ValueError("rows as a slice / range must have step 1 (a dense range); pass an index array otherwise")
        return (None, r.start, len(r)) if len(r) else (None, 0, 0)
    row_idx = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    return row_idx, 0, len(row_idx)


def _scan_args(panel, caller, cols, rows):
    """the opening of the resident-panel scans: the panel check, ``cols`` (None, or indices as contiguous int32) with their number,
    and ``rows`` as ``_row_selection`` gives them -- ``(ctx, cols, ncols, row_idx, row0, n_rows)``"""
    _need_resident_panel(panel, caller)
    if cols is None:
        ncols = panel.n_acc
    else:
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        ncols = len(cols)
    return (panel.ctx, cols, ncols) + _row_selection(panel, rows)


def _column_limit(ncols, limit, scan):
    """the library's limit on the columns of one call (``SNPM_<scan>_MAX_ACCESSIONS``), refused before numpy is asked for the result arrays"""
    if ncols > limit:
        raise AssertionError("too many accessions for one call: %d, at most %d (SNPM_%s_MAX_ACCESSIONS)" % (ncols, limit, scan))


KIN_MAX_ACCESSIONS = 11552     # SNPM_KIN_MAX_ACCESSIONS: columns of one ``kinship_counts`` call


def kinship_counts(panel, cols=None, rows=None):
    """Relatedness counts of every pair of accession columns of a resident panel in one device call
    (``snpm_panel_kinship_counts``).  ``cols``: accession indices, any order, repeats allowed (None: all accessions); ``rows``: panel
    rows as an index array, any order, repeats allowed, or a ``slice`` / ``range`` of step 1 (a dense range), or None (all rows).
    Returns ``(ninfo, same, diff)``, int32 [n_cols, n_cols], full and symmetric: rows where both calls are not missing, rows where
    both are homozygous and equal, rows where both are homozygous and different.  The reference's kinship is
    ``(same - diff) / ninfo``.  Only a panel whose columns all live on one device can be asked: group (accession-sharded) and
    streamed panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "kinship_counts", cols, rows)
    _column_limit(ncols, KIN_MAX_ACCESSIONS, "KIN")
    ninfo, same, diff = (np.empty((ncols, ncols), dtype=np.int32) for _ in range(3))
    check(ctx.lib.snpm_panel_kinship_counts(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(ninfo), ptr(same), ptr(diff)), ctx.h)
    return ninfo, same, diff


F1X_MAX_ACCESSIONS = 11552     # SNPM_F1X_MAX_ACCESSIONS: columns of one ``f1_counts`` call
F1X_NO_CLASS = 0xFF            # a row of the sample without a class: counted in ninfo only


def f1_counts(panel, sample_class, cols=None, rows=None):
    """The in-silico F1 of every pair of accession columns of a resident panel scored against one sample's hard calls, in one device
    call (``snpm_panel_f1_counts``).  ``sample_class``: uint8, one class per selected row -- 0 ref, 1 alt, 2 het, 0xFF none;
    ``cols`` / ``rows`` as for ``kinship_counts``.  Returns ``(hits, ninfo)``, int32 [n_cols, n_cols], full and symmetric: rows
    where the F1 of the two columns (ref where both are 0, alt where both are 1, het where both are called and differ) has the
    sample's class, and rows where it is informative at all.  With one-hot weights ``hits`` is the reference's score of the pair
    (core/csmatch.py:115-125) and ``ninfo`` its numinfo.  Group (accession-sharded) and streamed panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "f1_counts", cols, rows)
    sample_class = np.ascontiguousarray(sample_class, dtype=np.uint8).reshape(-1)
    assert len(sample_class) == n_rows, "one sample class per selected row: %d classes, %d rows" % (len(sample_class), n_rows)
    _column_limit(ncols, F1X_MAX_ACCESSIONS, "F1X")
    hits, ninfo = (np.empty((ncols, ncols), dtype=np.int32) for _ in range(2))
    check(ctx.lib.snpm_panel_f1_counts(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(sample_class), ptr(hits), ptr(ninfo)), ctx.h)
    return hits, ninfo


MIX_MAX_ACCESSIONS = 11552     # SNPM_MIX_MAX_ACCESSIONS: columns of one ``mix_counts`` call


def mix_counts(panel, alt, ref, cols=None, rows=None):
    """The read-count-weighted 2 x 2 table of every ordered pair of accession columns of a resident panel against one sample's
    allele depths, in one device call (``snpm_panel_mix_counts``).  ``alt`` / ``ref``: the sample's reads of the alt and of the ref
    allele at every selected row, 0 .. 255 each; ``cols`` / ``rows`` as for ``kinship_counts``.  Returns int32 [2, 2, 2, n_cols,
    n_cols]: ``table[w, ca, cb, a, b]`` is the sum, over the rows where column a has the homozygous call ca and column b the
    homozygous call cb, of the alt (w = 0) or ref (w = 1) reads; a het, "other" or missing call on either side drops the row for that
    pair.  ``table[w, ca, cb, a, b] == table[w, cb, ca, b, a]``; the diagonal holds the sums of every column on its own.  Group
    (accession-sharded) and streamed panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "mix_counts", cols, rows)
    counts = []
    for name, v in (("alt", alt), ("ref", ref)):
        v = np.asarray(v).reshape(-1)
        assert len(v) == n_rows, "one %s count per selected row: %d counts, %d rows" % (name, len(v), n_rows)
        assert v.dtype.kind in "iu" and (len(v) == 0 or (0 <= v.min() and v.max() <= 255)), "%s counts are integers 0 .. 255" % name
        counts.append(np.ascontiguousarray(v, dtype=np.uint8))
    _column_limit(ncols, MIX_MAX_ACCESSIONS, "MIX")
    table = np.empty((2, 2, 2, ncols, ncols), dtype=np.int32)
    check(ctx.lib.snpm_panel_mix_counts(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(counts[0]), ptr(counts[1]), ptr(table)), ctx.h)
    return table


def parent_counts(panel, sample_class, win_off, min_win_sites=1, cols=None, rows=None):
    """Every pair of accession columns of a resident panel scored, window by window, as the two parents of a recombinant sample (an
    F2, a backcross, a RIL with residual heterozygosity) against the sample's hard calls, in one device call
    (``snpm_panel_parent_counts``).  ``sample_class`` / ``cols`` / ``rows`` as for ``f1_counts``; ``win_off`` [n_win + 1]: offsets
    into the SELECTED rows (starts at 0, never decreases, ends at the row count; empty windows allowed); ``min_win_sites`` >= 1.
    Per cell (a, b) -- positions in the column list -- and window, over the rows where the F1 of the two columns is informative and
    the sample has a class: n such rows, of which hA / hB carry the sample's class in column a / b and hF in their F1.  A window
    with n < min_win_sites is not used; otherwise it adds max(hA, hB, hF) to the score and n to n_tot, and counts as the F1 (hF
    strictly the largest), or as the parent that fits better (a tie to the smaller position).  Returns ``(score, n_tot, w_first,
    w_het)``, int32 [n_cols, n_cols]: ``w_first[a, b]`` windows taken as column a, ``w_first[b, a]`` as column b, ``w_het`` as
    their F1.  Group (accession-sharded) and streamed panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "parent_counts", cols, rows)
    sample_class = np.ascontiguousarray(sample_class, dtype=np.uint8).reshape(-1)
    assert len(sample_class) == n_rows, "one sample class per selected row: %d classes, %d rows" % (len(sample_class), n_rows)
    win_off = np.ascontiguousarray(win_off, dtype=np.int64).reshape(-1)
    assert len(win_off) >= 1, "win_off holds n_win + 1 entries"
    _column_limit(ncols, F1X_MAX_ACCESSIONS, "F1X")
    score, n_tot, w_first, w_het = (np.empty((ncols, ncols), dtype=np.int32) for _ in range(4))
    check(ctx.lib.snpm_panel_parent_counts(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(sample_class), ptr(win_off), len(win_off) - 1,
                                           int(min_win_sites), ptr(score), ptr(n_tot), ptr(w_first), ptr(w_het)), ctx.h)
    return score, n_tot, w_first, w_het


IBD_COUNT_NAMES = ("w_used", "w_shared", "n_shared", "d_shared", "run_max", "n_runs", "w_in_runs")


def ibd_counts(panel, win_off, min_win_sites=20, max_diff_ppm=1000, min_run=1, cols=None, rows=None, bits=True):
    """For every pair of accession columns of a resident panel the windows in which the two are identical -- shared haplotype
    segments, identity by descent -- in one device call (``snpm_panel_ibd_counts``).  ``cols`` / ``rows`` as for
    ``kinship_counts``; ``win_off`` [n_win + 1]: offsets into the SELECTED rows (starts at 0, never decreases, ends at the row count;
    empty windows allowed).  Per cell (a, b) -- positions in the column list -- and window: n rows where both calls are homozygous,
    d of them where the two differ.  A window is used with n >= ``min_win_sites`` (>= 1), shared when used and
    d * 1 000 000 <= ``max_diff_ppm`` * n (0 .. 1 000 000), a break when used and not shared.  The windows of a call, in order, form
    runs: shared windows without a break between them (unused windows neither break a run nor count in it); a run is reported with
    ``min_run`` (>= 1) shared windows or more.  Returns a dict of ``w_used``, ``w_shared``, ``n_shared``, ``d_shared``, ``run_max``,
    ``n_runs``, ``w_in_runs`` -- int32 [n_cols, n_cols], full and symmetric -- and ``used_bits`` / ``shared_bits``, uint32 [n_cols,
    n_cols, ceil(n_win / 32)] (window w is bit w % 32 of word w // 32; None with ``bits=False``).  Group (accession-sharded) and
    streamed panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "ibd_counts", cols, rows)
    win_off = np.ascontiguousarray(win_off, dtype=np.int64).reshape(-1)
    assert len(win_off) >= 1, "win_off holds n_win + 1 entries"
    _column_limit(ncols, F1X_MAX_ACCESSIONS, "F1X")
    n_win = len(win_off) - 1
    out = {name: np.empty((ncols, ncols), dtype=np.int32) for name in IBD_COUNT_NAMES}
    out["used_bits"], out["shared_bits"] = ((np.empty((ncols, ncols, (n_win + 31) // 32), dtype=np.uint32) if bits else None) for _ in range(2))
    check(ctx.lib.snpm_panel_ibd_counts(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(win_off), n_win, int(min_win_sites),
                                        int(max_diff_ppm), int(min_run), *[ptr(out[name]) for name in IBD_COUNT_NAMES + ("used_bits", "shared_bits")]), ctx.h)
    return out


PCA_MAX_ACCESSIONS = 11552     # SNPM_PCA_MAX_ACCESSIONS: columns of one ``gram`` / ``loadings`` call
PCA_MAX_COMPONENTS = 32        # SNPM_PCA_MAX_COMPONENTS: columns of ``vec`` of one ``loadings`` call


def _class_table(tab, n_rows):
    tab = np.ascontiguousarray(tab, dtype=np.float64)
    assert tab.shape == (n_rows, 4), "one row of four class values per selected row: tab is %r, %d rows selected" % (tab.shape, n_rows)
    return tab


def gram(panel, tab, cols=None, rows=None):
    """The weighted Gram matrix of the accession columns of a resident panel over panel rows in one device call
    (``snpm_panel_gram``).  ``tab``: fp64 [n_rows, 4], for every selected row the value of a call with canonical code 0 (ref), 1
    (alt), 2 (het), 3 (an int8 panel's "other"); a missing call has value 0.  ``cols`` / ``rows`` as for ``kinship_counts``.
    Returns fp64 [n_cols, n_cols], ``sum_s t(s, i) t(s, j)``: full, symmetric bit for bit, not divided by the row count.  fp64 FMA
    in an order fixed by the arguments and ``SNPM_PCA_WS_MB``: the same call returns the same bits, and a table of small integers
    gives the exact integers.  A value of ``tab`` that is not finite is refused.  Group (accession-sharded) and streamed panels
    are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "gram", cols, rows)
    tab = _class_table(tab, n_rows)
    _column_limit(ncols, PCA_MAX_ACCESSIONS, "PCA")
    out = np.empty((ncols, ncols), dtype=np.float64)
    check(ctx.lib.snpm_panel_gram(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(tab), ptr(out)), ctx.h)
    return out


def loadings(panel, tab, vec, cols=None, rows=None):
    """``load[s, c] = sum_i t(s, i) vec[i, c]`` over the listed accession columns for every selected row of a resident panel, in one
    device call (``snpm_panel_loadings``): with the eigenvectors of the Gram matrix as ``vec`` the raw SNP loadings ``Z V``.
    ``tab`` / ``cols`` / ``rows`` as for ``gram``; ``vec``: fp64 [n_cols, k], 1 <= k <= 32, finite.  Returns fp64 [n_rows, k]."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "loadings", cols, rows)
    tab = _class_table(tab, n_rows)
    vec = np.ascontiguousarray(vec, dtype=np.float64)
    assert vec.ndim == 2 and vec.shape[0] == ncols, "vec is [n_cols, k]: got %r for %d columns" % (vec.shape, ncols)
    k = vec.shape[1]
    out = np.zeros((n_rows, k), dtype=np.float64)
    check(ctx.lib.snpm_panel_loadings(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(tab), ptr(vec), k, ptr(out)), ctx.h)
    return out


ADMIX_MAX_K = 16               # SNPM_ADMIX_MAX_K: components of one ``admix`` call
ADMIX_EPS = 1e-6               # SNPM_ADMIX_EPS: F stays inside [EPS, 1 - EPS]
ADMIX_UPDATE_F, ADMIX_UPDATE_Q = 1, 2
ADMIX_MAX_ITER = 10000         # iterations of one call


def admix(panel, Q, F, n_iter=1, cols=None, rows=None, update_q=True, update_f=True):
    """``n_iter`` joint EM iterations of the admixture model (STRUCTURE / FRAPPE / ADMIXTURE) on the accession columns of a resident
    panel in one device call (``snpm_panel_admix``).  ``Q``: fp64 [n_cols, K], the ancestry of every listed column, entries >= 0, rows
    summing to 1; ``F``: fp64 [n_rows, K], the alt frequency of every component at every selected row, inside [1e-6, 1 - 1e-6]; 1 <= K
    <= 16; ``cols`` / ``rows`` as for ``gram``.  Dosage 0 / 2 / 1 for ref / alt / het; a missing call and an int8 panel's "other"
    code contribute nothing.  Every iteration makes (Q', F') from the old pair, so the log-likelihood never decreases.  Returns
    (Q, F, loglik): new arrays -- the inputs are not written -- and fp64 [n_iter], ``loglik[t]`` the likelihood of the parameters at
    the START of iteration t.  With ``update_q=False`` / ``update_f=False`` that component comes back with its bits; with both False
    the call only evaluates the likelihood.  fp64 throughout in an order fixed by the arguments: the same call returns the same bits.
    Group (accession-sharded) and streamed panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "admix", cols, rows)
    Q, F = np.array(Q, dtype=np.float64, order="C"), np.array(F, dtype=np.float64, order="C")      # (copies: the call writes them)
    assert Q.ndim == 2 and Q.shape[0] == ncols, "Q is [n_cols, K]: got %r for %d columns" % (Q.shape, ncols)
    K = Q.shape[1]
    assert F.shape == (n_rows, K), "F is [n_rows, K]: got %r for %d rows and K = %d" % (F.shape, n_rows, K)
    n_iter = int(n_iter)
    loglik = np.zeros(max(n_iter, 0), dtype=np.float64)
    flags = (ADMIX_UPDATE_F if update_f else 0) | (ADMIX_UPDATE_Q if update_q else 0)
    check(ctx.lib.snpm_panel_admix(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, K, n_iter, flags, ptr(Q), ptr(F), ptr(loglik)), ctx.h)
    return Q, F, loglik


MK_MAX_ACCESSIONS = 4096       # SNPM_MK_MAX_ACCESSIONS: columns of one ``marker_select`` call
MK_NO_LIMIT = 2 ** 62           # ``max_markers=None``
MK_STOP_REASONS = ("all pairs resolved", "max_markers reached", "no eligible row with gain")


def marker_select(panel, depth=1, max_markers=None, coord=None, min_dist=0, eligible=None, cols=None, rows=None, first_gain=True):
    """A small set of rows (SNPs) of a resident panel that separates every pair of the listed accession columns ``depth`` times,
    chosen greedily on the device, all rounds in one call (``snpm_panel_marker_select``).  ``cols`` / ``rows`` as for
    ``kinship_counts``; a *position* is an index into the row selection.  A row separates a pair when both calls are homozygous and
    different.  Per round the eligible row that separates the most pairs still in need is picked (ties: the smallest position), the
    need of those pairs drops by one, and the pick becomes ineligible -- with ``coord`` (int64, one per selected row, any order) every
    row with ``|coord[r] - coord[pick]| < min_dist`` as well; ``eligible`` (one byte per selected row, 0 = never pick) masks rows from
    the start; ``max_markers`` (None: no limit) bounds the picks.  This is the textbook greedy set cover: not optimal, a smaller
    set may exist.  Returns a dict: ``chosen`` int64 [n_chosen] (positions, in pick order), ``gain_at`` int32 [n_chosen], ``n_chosen``,
    ``remaining`` (the sum of need over a < b), ``stop_reason`` (0 all pairs resolved, 1 ``max_markers`` reached, 2 no eligible row
    with gain: the cells of ``need`` > 0 are then the pairs the candidates cannot tell apart), ``need`` uint8 [n_cols, n_cols] and
    ``first_gain`` int32 [n_rows] (the pairs every row separates, whatever its eligibility; None with ``first_gain=False``; zeros from
    a call with fewer than two columns, no row or ``max_markers`` 0, which launches nothing).  Group (accession-sharded) and streamed
    panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "marker_select", cols, rows)
    _column_limit(ncols, MK_MAX_ACCESSIONS, "MK")
    max_markers = MK_NO_LIMIT if max_markers is None else int(max_markers)
    if coord is not None:
        coord = np.ascontiguousarray(coord, dtype=np.int64).reshape(-1)
        assert len(coord) == n_rows, "coord holds one entry per selected row"
    if eligible is not None:
        eligible = np.ascontiguousarray(np.asarray(eligible).reshape(-1) != 0, dtype=np.uint8)
        assert len(eligible) == n_rows, "eligible holds one entry per selected row"
    cap = max(0, min(max_markers, n_rows))
    chosen, gain_at = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int32)
    need = np.empty((ncols, ncols), dtype=np.uint8)
    first = np.empty(n_rows, dtype=np.int32) if first_gain else None
    n_chosen, remaining, reason = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    check(ctx.lib.snpm_panel_marker_select(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(coord), int(min_dist), ptr(eligible), int(depth),
                                           max_markers, ptr(chosen), ptr(gain_at), C.byref(n_chosen), C.byref(remaining), C.byref(reason), ptr(need),
                                           ptr(first)), ctx.h)
    n = int(n_chosen.value)
    return {"chosen": chosen[:n].copy(), "gain_at": gain_at[:n].copy(), "n_chosen": n, "remaining": int(remaining.value),
            "stop_reason": int(reason.value), "need": need, "first_gain": first}


SIM_MAX_ACCESSIONS = 11552     # SNPM_SIM_MAX_ACCESSIONS: columns of one ``sim_counts`` call
SIM_MAX_GROUPS = 64            # groups of one ``sim_counts`` call


def sim_err_threshold(err_rate):
    """the library's ``err_thr`` of an error rate in [0, 1]: floor(err_rate * 2^32)"""
    err_rate = float(err_rate)
    if not 0.0 <= err_rate <= 1.0:
        raise ValueError("err_rate must lie in 0 .. 1: got %r" % (err_rate,))
    return int(np.floor(err_rate * 4294967296.0))


def sim_counts(panel, grp_off, err_rate, seed, cols=None, rows=None):
    """The sample SIMULATED from every accession column of a resident panel -- its calls at the selected rows, each replaced with
    probability ``err_rate`` by a class drawn from 0 / 1 / 2 by a counter-based hash of (``seed``, position of the column in the list,
    position of the row in the selection) -- scored against every accession column, per group of selected rows, in one device call
    (``snpm_panel_sim_counts``).  ``grp_off`` [n_grp + 1]: offsets into the SELECTED rows (starts at 0, never decreases, ends at the
    row count; empty groups allowed; at most 64 groups); ``cols`` / ``rows`` as for ``kinship_counts``.  Returns ``(score, ninfo)``,
    int32 [n_grp, n_cols, n_cols], NOT symmetric: ``ninfo[g, a, b]`` rows of group g where sample a has a call and column b's is not
    missing, ``score[g, a, b]`` rows where column b's code is sample a's class -- the reference's NumInfoSites / ScoreList of that
    sample against b.  Group (accession-sharded) and streamed panels are refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "sim_counts", cols, rows)
    grp_off = np.ascontiguousarray(grp_off, dtype=np.int64).reshape(-1)
    assert len(grp_off) >= 1, "grp_off holds n_grp + 1 entries"
    n_grp = len(grp_off) - 1
    err_thr = sim_err_threshold(err_rate)
    seed = int(seed) % (1 << 64)
    _column_limit(ncols, SIM_MAX_ACCESSIONS, "SIM")
    if not 1 <= n_grp <= SIM_MAX_GROUPS or n_grp * ncols * ncols >= 1 << 31:
        check(ctx.lib.snpm_panel_sim_counts(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(grp_off), n_grp, err_thr, seed, None, None), ctx.h)
    score, ninfo = (np.empty((n_grp, ncols, ncols), dtype=np.int32) for _ in range(2))
    check(ctx.lib.snpm_panel_sim_counts(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(grp_off), n_grp, err_thr, seed, ptr(score), ptr(ninfo)), ctx.h)
    return score, ninfo


MOS_MAX_ACCESSIONS = 12288     # SNPM_MOS_MAX_ACCESSIONS: columns (states) of one ``mosaic`` call
MOS_SWITCH_MAX = 1 << 20       # the largest switch cost


def mosaic(panel, classes, chain_off, cost, switch_cost, cols=None, rows=None, want_col_cost=False):
    """Samples as MOSAICS of the accession columns of a resident panel: the copying-model Viterbi with a uniform switch cost and
    integer costs, the states being all the listed columns, for every (chain, sample) in one device call (``snpm_panel_mosaic``;
    include/snpmatch_hip.h states the model).  ``classes``: uint8 [n_samples, n_rows] (or [n_rows], one sample), per selected row
    0 ref, 1 alt, 2 het, 0xFF none; ``chain_off`` [n_chain + 1]: offsets into the SELECTED rows (starts at 0, never decreases, ends
    at the row count; a chain is a chromosome; empty chains allowed); ``cost`` [3, 4]: entries 0 .. 15, indexed [sample class][DB
    code 0, 1, 2, 3]; ``switch_cost`` 1 .. 2^20; ``cols`` / ``rows`` as for ``kinship_counts``.  Returns ``(state, chain_cost,
    col_cost)``: int32 [n_samples, n_rows] positions in the column list, int32 [n_samples, n_chain], and int32 [n_samples, n_chain,
    n_cols] -- the cost of never switching -- or None without ``want_col_cost``.  Group (accession-sharded) and streamed panels are
    refused."""
    ctx, cols, ncols, row_idx, row0, n_rows = _scan_args(panel, "mosaic", cols, rows)
    classes = np.ascontiguousarray(classes, dtype=np.uint8)
    if classes.ndim == 1:
        classes = classes.reshape(1, -1)
    assert classes.ndim == 2 and classes.shape[1] == n_rows, "one class per sample and selected row: classes %s, %d rows" % (classes.shape, n_rows)
    n_samples = classes.shape[0]
    chain_off = np.ascontiguousarray(chain_off, dtype=np.int64).reshape(-1)
    assert len(chain_off) >= 1, "chain_off holds n_chain + 1 entries"
    n_chain = len(chain_off) - 1
    cost = np.ascontiguousarray(cost)
    assert cost.shape == (3, 4), "cost is [3, 4]: [sample class][DB code]"
    assert cost.dtype.kind in "iu" and cost.min() >= 0 and cost.max() <= 255, "cost holds small non-negative integers"
    cost = cost.astype(np.uint8)
    switch_cost = int(switch_cost)
    if not -2 ** 31 <= switch_cost < 2 ** 31:
        raise AssertionError("switch_cost must be 1 .. 2^20")
    _column_limit(ncols, MOS_MAX_ACCESSIONS, "MOS")
    state = np.empty((n_samples, n_rows), dtype=np.int32)
    chain_cost = np.empty((n_samples, n_chain), dtype=np.int32)
    col_cost = np.empty((n_samples, n_chain, ncols), dtype=np.int32) if want_col_cost else None
    check(ctx.lib.snpm_panel_mosaic(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, ptr(chain_off), n_chain, ptr(classes), n_samples,
                                    ptr(cost), switch_cost, ptr(state), ptr(chain_cost), ptr(col_cost)), ctx.h)
    return state, chain_cost, col_cost


SITE_MAX_GROUPS = 32           # SNPM_SITE_MAX_GROUPS: groups of one ``snpm_panel_site_counts`` call


def _site_layers(cols):
    """A column list as layers of DISTINCT columns: layer j holds the columns listed more than j times (ascending).  A list without
    repeats is one layer; an empty list is one empty layer."""
    cols = np.asarray(cols).reshape(-1)
    if cols.dtype.kind not in "iu" and len(cols):
        raise TypeError("accession indices must be integers, got %s" % cols.dtype)
    uniq, times = np.unique(cols.astype(np.int64), return_counts=True)
    if len(uniq) and (uniq[0] < -2 ** 31 or uniq[-1] >= 2 ** 31):
        raise AssertionError("accession index outside the panel")
    return [uniq[times > j].astype(np.int32) for j in range(int(times.max()) if len(times) else 1)]


def _site_counts_call(panel, col_lists, row_idx, row0, n_rows):
    """one ``snpm_panel_site_counts`` call: ``col_lists`` is None (one group of all accessions) or at most SITE_MAX_GROUPS lists of
    distinct columns.  int32 [groups, n_rows, 4]."""
    n_groups = 1 if col_lists is None else len(col_lists)
    out = np.empty((n_groups, n_rows, 4), dtype=np.int32)
    cols = off = None
    if col_lists is not None:
        off = np.zeros(n_groups + 1, dtype=np.int64)
        np.cumsum([len(c) for c in col_lists], out=off[1:])
        cols = np.ascontiguousarray(np.concatenate(col_lists) if col_lists else np.zeros(0), dtype=np.int32)
    check(panel.ctx.lib.snpm_panel_site_counts(panel.h, ptr(cols), ptr(off), n_groups, ptr(row_idx), row0, n_rows, ptr(out)), panel.ctx.h)
    return out


def site_counts(panel, groups=None, rows=None):
    """Allele counts of every selected panel row per group of accession columns, one streaming pass over the resident panel for
    up to SITE_MAX_GROUPS groups (``snpm_panel_site_counts``).  ``groups``: None (one group of all accessions), one index array
    (one group) or a list of index arrays; groups may overlap and may be empty, and a column that a group lists k times counts k
    times, as numpy fancy indexing would (the device takes a column once per group: such a group travels as k layers of distinct
    columns, layer j = the columns listed more than j times, and the layers' counts are added here).  ``rows``: panel rows as an
    index array, any order, repeats allowed, or a ``slice`` / ``range`` of step 1 (a dense range), or None (all rows).
    Returns int32 [G, n_rows, 4]: per group and row c0, c1, c2 (members with code 0 / 1 / 2) and ninfo (members with a call; an
    int8 panel's code 3 is informative and in none of c0..c2).  More groups (layers) than SITE_MAX_GROUPS take several calls.
    Only a panel whose columns all live on one device can be asked: group (accession-sharded) and streamed panels are refused."""
    _need_resident_panel(panel, "site_counts")
    row_idx, row0, n_rows = _row_selection(panel, rows)
    if groups is None:
        return _site_counts_call(panel, None, row_idx, row0, n_rows)
    if isinstance(groups, np.ndarray) or (len(groups) and np.isscalar(groups[0])):
        groups = [groups]
    layers, owner = [], []
    for g, cols in enumerate(groups):
        for layer in _site_layers(cols):
            layers.append(layer)
            owner.append(g)
    out = np.zeros((len(groups), n_rows, 4), dtype=np.int32)
    for at in range(0, len(layers), SITE_MAX_GROUPS):
        part = _site_counts_call(panel, layers[at:at + SITE_MAX_GROUPS], row_idx, row0, n_rows)
        np.add.at(out, owner[at:at + SITE_MAX_GROUPS], part)
    return out


LD_MAX_BAND = 4096             # SNPM_LD_MAX_BAND: offsets of one ``snpm_panel_ld_band`` call


def ld_slab_rows(ws_bytes, n_acc, band, n_rows):
    """rows of one slab of an ``ld_band`` call under a workspace budget of ``ws_bytes`` (SNPM_LD_WS_MB): ``ld_slab_rows`` of
    csrc/snpm_k_ld.hpp in Python, for tools and tests that want the plan (the host driver of the kernel prints the library's)"""
    words = (n_acc + 31) // 32
    per_row, halo = band * 44 + words * 12, band * words * 12
    fit = (ws_bytes - halo) // per_row // 64 * 64 if ws_bytes > halo else 0
    return min(max(fit, 64), n_rows)


def ld_band(panel, band, cols=None, rows=None, v_alt=2, v_het=1, min_n=2, counts=True, r2=True):
    """Linkage disequilibrium of every selected row of a resident panel with each of the ``band`` rows after it, in one device call
    (``snpm_panel_ld_band``).  ``cols``: distinct accession indices, any order (None: all accessions; a repeat is refused);
    ``rows``: panel rows as an index array, any order, repeats allowed, or a ``slice`` / ``range`` of step 1 (a dense range), or
    None (all rows): row k of the SELECTION is paired with rows k + 1 .. k + band of it.  Returns ``(counts, r2)``: int32
    [n_rows, band, 9] -- n, Ak, Hk, Aj, Hj, AA, AH, HA, HH over the selected columns (a = code 1, h = code 2, m = code 0 / 1 / 2) --
    and fp64 [n_rows, band], the squared correlation of the genotype values (``v_alt`` for code 1, ``v_het`` for code 2; both
    0..3), nan where fewer than ``min_n`` columns are informative in both rows or a row is constant among them.  Cells with k + d >=
    n_rows are zero / nan.  ``counts=False`` / ``r2=False``: that array is not computed and None comes back in its place.  Only a
    panel whose columns all live on one device can be asked: group (accession-sharded) and streamed panels are refused."""
    _need_resident_panel(panel, "ld_band")
    for name, v in (("band", band), ("v_alt", v_alt), ("v_het", v_het), ("min_n", min_n)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise TypeError("%s must be an integer, got %r" % (name, v))
    if not 1 <= band <= LD_MAX_BAND:
        raise AssertionError("band must be 1 .. %d (SNPM_LD_MAX_BAND), got %d" % (LD_MAX_BAND, band))
    if not (counts or r2):
        raise ValueError("ld_band: neither counts nor r2 wanted")
    ncols = 0
    if cols is not None:
        cols = np.asarray(cols).reshape(-1)
        if cols.dtype.kind not in "iu" and len(cols):
            raise TypeError("accession indices must be integers, got %s" % cols.dtype)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        ncols = len(cols)
    row_idx, row0, n_rows = _row_selection(panel, rows)
    out_c = np.empty((n_rows, band, 9), dtype=np.int32) if counts else None
    out_r = np.empty((n_rows, band), dtype=np.float64) if r2 else None
    check(panel.ctx.lib.snpm_panel_ld_band(panel.h, ptr(cols), ncols, ptr(row_idx), row0, n_rows, band, v_alt, v_het, min_n, ptr(out_c),
                                           ptr(out_r)), panel.ctx.h)
    return out_c, out_r


def ld_prune(r2, eligible=None, threshold=0.2):
    """Greedy marker pruning on a band of r2 values [n_rows, band] as ``ld_band`` returns it (``snpm_ld_prune``, host code): bool
    [n_rows], row k kept when it is eligible (None: every row) and no kept row j of the ``band`` rows before it has
    ``r2[j, k - j - 1] > threshold``.  nan never prunes."""
    r2 = np.ascontiguousarray(r2, dtype=np.float64)
    if r2.ndim != 2 or r2.shape[1] < 1:
        raise ValueError("r2 must be [n_rows, band] with band >= 1, got shape %r" % (r2.shape,))
    if eligible is not None:
        eligible = np.ascontiguousarray(np.asarray(eligible).astype(bool).reshape(-1)).view(np.uint8)
        if len(eligible) != len(r2):
            raise ValueError("eligible must have one entry per row of r2")
    keep = np.zeros(len(r2), dtype=np.uint8)
    rc = _lib.load().snpm_ld_prune(len(r2), r2.shape[1], ptr(r2), ptr(eligible), float(threshold), ptr(keep))
    if rc:
        raise AssertionError("snpm_ld_prune refused its arguments (%d)" % rc)
    return keep.astype(bool)


WIN_MAX_ACCESSIONS = 65535 * 64     # SNPM_WIN_MAX_ACCESSIONS: columns of one ``snpm_panel_window_counts`` call (the plane kernel's grid)
WIN_STEP_ROWS = 1024                # rows of a plane step of ``k_win_planes``: a slab is whole steps


def window_slabs(ws_bytes, ncols, cells_per_window, win_off, n_rows):
    """the slabs of a ``window_counts`` call under a workspace budget of ``ws_bytes`` (SNPM_WIN_WS_MB) as ``(s0, steps, w_lo, n_w)``:
    ``win_slab_steps`` of csrc/snpm_k_win.hpp in Python, for tools and tests that want the plan (the host driver of the kernel prints
    the library's).  ``cells_per_window``: the columns plus the pairs asked for."""
    win_off = [int(v) for v in win_off]
    n_win = len(win_off) - 1
    step_bytes, cell_bytes = 4 * (-(-ncols // 64) * 64) * 16 * 8, 16 * cells_per_window
    out, s0, w_lo = [], 0, 0
    while s0 < n_rows:
        while w_lo < n_win - 1 and win_off[w_lo + 1] <= s0:
            w_lo += 1
        need, steps, w_end = -(-(n_rows - s0) // WIN_STEP_ROWS), 0, w_lo
        while True:
            s1, e = min(s0 + (steps + 1) * WIN_STEP_ROWS, n_rows), w_end
            while e < n_win and win_off[e] < s1:
                e += 1
            if steps >= 1 and (steps + 1) * step_bytes + (e - w_lo) * cell_bytes > ws_bytes:
                break
            steps, w_end = steps + 1, e
            if steps >= need:
                break
        out.append((s0, steps, w_lo, w_end - w_lo))
        s0 += steps * WIN_STEP_ROWS
    return out


def window_counts(panel, win_off, cols=None, pairs=None, rows=None, acc_counts=True):
    """Per genome window, the call counts of every listed accession column and the agreement counts of listed pairs of columns of
    a resident panel, in one device call (``snpm_panel_window_counts``).  ``rows``: panel rows as an index array, any order, repeats
    allowed, or a ``slice`` / ``range`` of step 1 (a dense range), or None (all rows); ``win_off`` [n_win + 1]: offsets into the
    SELECTED rows, starting at 0, never decreasing, ending at their number -- window w holds the selected rows ``win_off[w] ..
    win_off[w + 1] - 1``, empty windows are allowed.  ``cols``: accession indices, any order, repeats allowed (None: all);
    ``pairs``: int [n_pairs, 2], indices INTO THE COLUMN LIST (``(a, a)`` and both orders of a pair are allowed), or None.
    Returns ``(acc, pair)``: int32 [n_win, n_cols, 4] -- c0, c1, c2 (rows with code 0 / 1 / 2) and ninfo (rows with a call; an int8
    panel's code 3 is informative and in none of c0..c2) -- or None with ``acc_counts=False``, and int32 [n_pairs, n_win, 4] -- n
    (both calls 0 / 1 / 2), eq (equal codes among them), hom_same, hom_diff (both homozygous, equal / different) -- or None without
    ``pairs``.  Only a panel whose columns all live on one device can be asked: group (accession-sharded) and streamed panels are
    refused."""
    _need_resident_panel(panel, "window_counts")
    if cols is None:
        ncols = panel.n_acc
    else:
        cols = np.asarray(cols).reshape(-1)
        if cols.dtype.kind not in "iu" and len(cols):
            raise TypeError("accession indices must be integers, got %s" % cols.dtype)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        ncols = len(cols)
    _column_limit(ncols, WIN_MAX_ACCESSIONS, "WIN")
    pa = pb = None
    n_pairs = 0
    if pairs is not None:
        pairs = np.asarray(pairs)
        if pairs.dtype.kind not in "iu" and pairs.size:
            raise TypeError("pairs must be integer indices into the column list, got %s" % pairs.dtype)
        pairs = pairs.reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0], dtype=np.int32), np.ascontiguousarray(pairs[:, 1], dtype=np.int32)
        n_pairs = len(pa)
    if not acc_counts and pairs is None:
        raise ValueError("window_counts: neither acc_counts nor pairs wanted")
    win_off = np.ascontiguousarray(win_off, dtype=np.int64).reshape(-1)
    n_win = len(win_off) - 1
    if n_win < 0:
        raise ValueError("win_off holds n_win + 1 entries")
    row_idx, row0, n_rows = _row_selection(panel, rows)
    out_a = np.zeros((n_win, ncols, 4), dtype=np.int32) if acc_counts else None
    out_p = np.zeros((n_pairs, n_win, 4), dtype=np.int32) if pairs is not None else None
    check(panel.ctx.lib.snpm_panel_window_counts(panel.h, ptr(cols), ncols, ptr(pa), ptr(pb), n_pairs, ptr(row_idx), row0, n_rows,
                                                 ptr(win_off), n_win, ptr(out_a), ptr(out_p)), panel.ctx.h)
    return out_a, out_p


def weight_codes(wei, table):
    """uint16 codes [n, 3] with table[codes] == wei bit for bit, or None when some weight is not in ``table``
    (float64 [<= 65536], e.g. ``pl_table()``).  A binary search per weight on the host; parsers that still hold the
    integer PLs produce the codes directly instead (code = PL)."""
    wei = np.ascontiguousarray(wei, dtype=np.float64)
    order = np.argsort(table, kind="stable")
    pos = np.searchsorted(table[order], wei.ravel())
    pos[pos >= len(order)] = len(order) - 1
    codes = order[pos].astype(np.uint16)
    if not np.array_equal(table[codes].view(np.uint64), wei.ravel().view(np.uint64)):
        return None
    return codes.reshape(wei.shape)


def pl_table(n=8192):
    """table[k] = exp(-k / 10) for PL k = 0 .. n - 1 as numpy rounds it (what ParseInputs computes from a VCF's PL field,
    core/parsers.py:147-150).  exp underflows to exactly 0.0 from k = 7451 on, so the last entries double as the zeros
    of hard-call rows (code n - 1)."""
    return np.exp(np.arange(n, dtype=np.float64) / (-10))


def score_batch(panel, samples, chunk=1000, skip_hets=False, mode=MODE_EXACT, likelihoods=True, device=None, table=None, out=None):
    """Many samples against one resident panel in one call (snpm_score_batch).  ``samples``: list of
    (row_idx int64 [n_b], wei float64 [n_b, 3]) pairs.  With ``table`` (float64 [256]) the second element of a sample is
    uint16 codes [n_b, 3] instead, wei = table[codes] (snpm_score_batch_coded: 10 instead of 32 bytes per SNP over PCIe).  ``device`` = (d_row_idx, d_wei, offsets): the concatenated
    inputs already in device memory (raw pointers) instead.  Returns a dict with score / ninfo (and lik / lrt)
    arrays [B, n_acc] and the re-evaluation counters.  ``out``: the dict of an earlier call of the same shape, whose arrays are
    written again instead of new ones (a service that scores batch after batch: fresh arrays cost their page faults on every
    call, 9 MB of them for 256 samples x 1135 accessions)."""
    if isinstance(panel, GroupPanel):
        return panel.score_batch(samples, chunk, skip_hets, mode, likelihoods, device, table)
    ctx = panel.ctx
    wdtype = np.float64 if table is None else np.uint16
    if device is None and isinstance(samples, tuple):
        # already concatenated: (row_idx int64 [N], wei float64 [N, 3] (or codes uint8 [N, 3]), offsets int64 [B + 1])
        rows, wei, off = samples
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        wei = np.ascontiguousarray(wei, dtype=wdtype)
        off = np.ascontiguousarray(off, dtype=np.int64)
        assert wei.ndim == 2 and wei.shape[1] == 3 and len(rows) == len(wei) == off[-1]
        p_rows, p_wei, dev_flag = ptr(rows), ptr(wei), 0
    elif device is None:
        off = np.zeros(len(samples) + 1, dtype=np.int64)
        for b, (rows, wei) in enumerate(samples):
            wei = np.asarray(wei)
            assert wei.ndim == 2 and wei.shape[1] == 3, "SNP weights should be a np.array with  shape == n,3"
            assert len(rows) == wei.shape[0], "please provide same number of positions for both sample and db"
            off[b + 1] = off[b] + len(rows)
        rows = np.ascontiguousarray(np.concatenate([np.asarray(s[0], dtype=np.int64) for s in samples]) if samples
                                    else np.zeros(0, dtype=np.int64))
        wei = np.ascontiguousarray(np.concatenate([np.asarray(s[1], dtype=wdtype) for s in samples]) if samples
                                   else np.zeros((0, 3), dtype=wdtype))
        p_rows, p_wei, dev_flag = ptr(rows), ptr(wei), 0
    else:
        d_rows, d_wei, off = device
        off = np.ascontiguousarray(off, dtype=np.int64)
        p_rows, p_wei, dev_flag = C.c_void_p(int(d_rows)), C.c_void_p(int(d_wei)), 1
    nb, na = len(off) - 1, panel.n_acc
    reuse = out
    out = {}
    for key, dtype in (("score", np.float64), ("ninfo", np.int64)) + ((("lik", np.float64), ("lrt", np.float64)) if likelihoods else ()):
        arr = reuse.get(key) if reuse is not None else None
        if not (isinstance(arr, np.ndarray) and arr.shape == (nb, na) and arr.dtype == dtype and arr.flags.c_contiguous and arr.flags.writeable):
            arr = np.empty((nb, na), dtype=dtype)
        out[key] = arr
    info = np.zeros(4, dtype=np.int64)
    if table is not None:
        assert device is None, "coded weights come from host memory"
        table = np.ascontiguousarray(table, dtype=np.float64)
        assert table.ndim == 1 and 1 <= len(table) <= 65536
        check(ctx.lib.snpm_score_batch_coded(panel.h, nb, ptr(off), p_rows, p_wei, ptr(table), len(table), int(chunk), int(bool(skip_hets)),
                                             int(mode), ptr(out["score"]), ptr(out["ninfo"]), ptr(out.get("lik")),
                                             ptr(out.get("lrt")), ptr(info)), ctx.h)
    else:
        check(ctx.lib.snpm_score_batch(panel.h, nb, ptr(off), p_rows, p_wei, dev_flag, int(chunk), int(bool(skip_hets)), int(mode),
                                       ptr(out["score"]), ptr(out["ninfo"]), ptr(out.get("lik")), ptr(out.get("lrt")), ptr(info)),
              ctx.h)
    out["pairs_reeval"], out["strict_fallback"] = int(info[0]), bool(info[1])
    out["shared_rows"], out["union_rows"] = bool(info[2]), int(info[3])
    return out


SHARED_WHY_NOT = {0: "", 1: "policy", 2: "too few samples or rows", 3: "a row list is not strictly increasing", 4: "a weight outside [0, 1]",
                  5: "call codes > 2 in the panel", 6: "overlap below the threshold", 7: "sizes beyond 32-bit indices", 8: "a row index outside the panel"}


def batch_configure(ctx, shared_rows=-1, digits=0, min_density=-1.0):
    """Policy of score_batch for batches whose samples share DB rows (snpm_batch_configure): shared_rows -1 automatic (device
    inputs, >= 4 samples, enough overlap), 0 never, 1 whenever the batch allows it; digits 3..7 base-256 digits of the fixed-point
    weights (-1: chosen by the longest sample, 0: keep); min_density: threshold of the automatic choice (negative: keep)."""
    check(ctx.lib.snpm_batch_configure(ctx.h, int(shared_rows), int(digits), float(min_density)), ctx.h)


def batch_last_stats(ctx):
    """What the context's last score_batch call did about shared rows (snpm_batch_last_stats)."""
    st = np.zeros(8, dtype=np.int64)
    check(ctx.lib.snpm_batch_last_stats(ctx.h, ptr(st)), ctx.h)
    return {"taken": bool(st[0]), "why_not": SHARED_WHY_NOT.get(int(st[1]), str(int(st[1]))), "union_rows": int(st[2]),
            "density": float(st[3]) / 1e6, "row_tiles": int(st[4]), "groups": int(st[5]), "passes": int(st[6]), "digits": int(st[7])}


class Carry(object):
    """Running per-accession totals of a job scored SNP slab after SNP slab (include/snpmatch_hip.h, snpm_carry_*)."""

    def __init__(self, ctx, n_acc):
        self.ctx, self.n_acc = ctx, int(n_acc)
        h = C.c_void_p()
        check(ctx.lib.snpm_carry_create(ctx.h, self.n_acc, C.byref(h)), ctx.h)
        self.h = h
        ctx._children.add(self)

    def reset(self):
        check(self.ctx.lib.snpm_carry_reset(self.h), self.ctx.h)

    def bind_outputs(self, d_score, d_ninfo):
        """keep the totals in caller-owned device buffers (raw pointers of float64 [n_acc] / int64 [n_acc])"""
        check(self.ctx.lib.snpm_carry_bind_outputs(self.h, C.c_void_p(d_score) if d_score else None,
                                                   C.c_void_p(d_ninfo) if d_ninfo else None), self.ctx.h)

    def set_columns(self, cols):
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        check(self.ctx.lib.snpm_carry_set_columns(self.h, ptr(cols), len(cols)), self.ctx.h)

    def finish(self, want_results=True):
        """(score, ninfo, flagged accessions): flagged is empty unless the job ran in MODE_EXACT and some totals could
        not be certified; len(flagged) > 64 is reported as a count only (``n_flagged``)."""
        score = np.empty(self.n_acc, dtype=np.float64) if want_results else None
        ninfo = np.empty(self.n_acc, dtype=np.int64) if want_results else None
        cols = np.zeros(64, dtype=np.int32)
        nf = C.c_int64(0)
        check(self.ctx.lib.snpm_carry_finish(self.h, ptr(score), ptr(ninfo), ptr(cols), 64, C.byref(nf)), self.ctx.h)
        self.n_flagged = nf.value
        return score, ninfo, np.sort(cols[:min(nf.value, 64)])

    def error_bound(self):
        """bound on |total - reference total| of the slabs scored so far in MODE_EXACT (0 for all-integer jobs)"""
        b = C.c_double(0)
        check(self.ctx.lib.snpm_carry_error_bound(self.h, C.byref(b)), self.ctx.h)
        return b.value

    def patch_from(self, cols_carry):
        check(self.ctx.lib.snpm_carry_patch(self.h, cols_carry.h), self.ctx.h)

    def device_ptrs(self):
        ds, dn = C.c_void_p(), C.c_void_p()
        check(self.ctx.lib.snpm_carry_device_ptrs(self.h, C.byref(ds), C.byref(dn)), self.ctx.h)
        return ds.value, dn.value

    def free(self):
        if self.h:
            if self.ctx.h:
                self.ctx.lib.snpm_carry_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SlabScorer(object):
    """Genotyper.genotyper over a SNP axis that does not fit in HBM (core/snpmatch.py:207-233 for a panel scored slab
    by slab).  ``slabs`` is a list of row counts; ``load(k, panel)`` must leave slab k in rows [0, slabs[k]) of
    ``panel`` (upload, file, generator); ``weights(k)`` returns the float64 [slabs[k], 3] weights of its rows (a numpy
    array, or a raw device pointer when ``device_weights``).  Every slab but the last holds a multiple of ``chunk``
    rows.  ``run`` returns (ScoreList, NumInfoSites, info); in MODE_EXACT the accessions whose total the certificate
    cannot vouch for are re-scored in reference order by streaming the slabs a second time."""

    def __init__(self, panel, slabs, load, weights, chunk=1000, skip_hets=False, device_weights=False):
        self.panel, self.slabs, self.load, self.weights = panel, [int(s) for s in slabs], load, weights
        self.chunk, self.skip, self.device_weights = int(chunk), bool(skip_hets), device_weights
        assert all(s % self.chunk == 0 for s in self.slabs[:-1]), "every slab but the last must hold a multiple of chunk rows"
        assert max(self.slabs) <= panel.n_snp
        self.queries = [None] * len(self.slabs)         # kept: a second pass reuses them
        self.carry = Carry(panel.ctx, panel.n_acc)

    def _query(self, k):
        if self.queries[k] is None:
            w = self.weights(k)
            self.queries[k] = (Query.from_device(self.panel, None, w, self.slabs[k]) if self.device_weights
                               else Query(self.panel, None, w))
        return self.queries[k]

    def _after(self, k):
        return sum(-(-s // self.chunk) for s in self.slabs[k + 1:])

    def _pass(self, carry, mode):
        for k in range(len(self.slabs)):
            self.load(k, self.panel)
            self._query(k).run_carry(carry, self.chunk, self.skip, mode, self._after(k))

    def run(self, mode=MODE_EXACT):
        self.carry.reset()
        self._pass(self.carry, mode)
        score, ninfo, flagged = self.carry.finish()
        info = {"n_strict_reeval": int(self.carry.n_flagged), "second_pass": False}
        if self.carry.n_flagged > 0:
            info["second_pass"] = True
            if self.carry.n_flagged <= 64:
                cols = Carry(self.panel.ctx, self.panel.n_acc)
                cols.set_columns(flagged)
                self._pass(cols, MODE_STRICT)
                self.carry.patch_from(cols)
                cols.free()
            else:                                   # many exact-integer totals: everything in reference order
                self.carry.reset()
                self._pass(self.carry, MODE_STRICT)
            score, ninfo, _ = self.carry.finish()
        return score, ninfo, info

    def free(self):
        for q in self.queries:
            if q is not None:
                q.free()
        self.carry.free()


# ----------------------------------------------------------------------------------------------------------
# Several GPUs: accession shards + ONE RCCL all-gather of the per-accession results, behind the C ABI
# (include/snpmatch_hip.h, snpm_group_*).  Reference: accession columns never interact (core/snpmatch.py:84-88); the
# likelihood step needs the minimum over all accessions (core/snpmatch.py:112).
class Group(object):
    """The GPUs of one job.  ``Group.local([0, 1, ...])``: this process drives all of them (ncclCommInitAll, no launcher);
    ``Group.from_rank(ctx, id_bytes, world, rank)``: one process per GPU (``Group.unique_id()`` on rank 0, handed to the
    other ranks by the caller).  ``loopback=True`` replaces RCCL by device-to-device copies: a test transport that also
    takes one device several times."""

    def __init__(self, handle, contexts, owns_contexts):
        self.lib = _lib.load()
        self.h = handle
        self.contexts = contexts
        self._owns_contexts = owns_contexts
        w, r0, nl = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check_group(self.lib.snpm_group_info(self.h, C.byref(w), C.byref(r0), C.byref(nl)), self.h)
        self.world, self.rank0, self.n_local = w.value, r0.value, nl.value
        ref = weakref.ref(self)
        self._atexit = lambda: (ref() is not None) and ref().free()
        atexit.register(self._atexit)

    @staticmethod
    def unique_id():
        lib = _lib.load()
        buf = C.create_string_buffer(_lib.GROUP_ID_BYTES)
        _lib.check_group(lib.snpm_group_unique_id(buf), None)
        return buf.raw

    @classmethod
    def local(cls, device_ids, loopback=False):
        lib = _lib.load()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        h = C.c_void_p()
        _lib.check_group(lib.snpm_group_create_local(ids, len(device_ids), _lib.GROUP_LOOPBACK if loopback else 0, C.byref(h)), None)
        ctxs = []
        for i, d in enumerate(device_ids):
            ch = C.c_void_p()
            _lib.check_group(lib.snpm_group_ctx(h, i, C.byref(ch)), h)
            ctxs.append(Context(d, _borrowed=ch))
        return cls(h, ctxs, True)

    @classmethod
    def from_rank(cls, ctx, id_bytes, world, rank):
        lib = _lib.load()
        assert len(id_bytes) == _lib.GROUP_ID_BYTES
        h = C.c_void_p()
        _lib.check_group(lib.snpm_group_create_rank(ctx.h, C.c_char_p(bytes(id_bytes)), int(world), int(rank), C.byref(h)), None)
        return cls(h, [ctx], False)

    @property
    def transport(self):
        return (self.lib.snpm_group_transport(self.h) or b"").decode()

    def shard(self, n_acc, rank):
        a0, a1 = C.c_int64(0), C.c_int64(0)
        _lib.check_group(self.lib.snpm_group_shard(self.h, int(n_acc), int(rank), C.byref(a0), C.byref(a1)), self.h)
        return a0.value, a1.value

    def local_shards(self, n_acc):
        return [self.shard(n_acc, self.rank0 + i) for i in range(self.n_local)]

    def gather(self, d_scores, d_ninfos, n_acc, m=1, in_ld=None, truncate=False, host=True, likelihoods=False):
        """ONE all-gather of the members' shard results (raw device pointers, one per local member): returns host arrays
        score / ninfo [n_acc] ([m, n_acc] for m > 1) (+ lik, lrt); ``host=False``: nothing is copied or waited for, the
        gathered vectors stay on the devices (``gathered_ptrs``)."""
        n_acc, m = int(n_acc), int(m)
        if in_ld is None:
            in_ld = max(a1 - a0 for a0, a1 in self.local_shards(n_acc))
        ps = (C.c_void_p * self.n_local)(*[C.c_void_p(int(p or 0)) for p in d_scores])
        pn = (C.c_void_p * self.n_local)(*[C.c_void_p(int(p or 0)) for p in d_ninfos])
        shape = (n_acc,) if m == 1 else (m, n_acc)
        out = {}
        if host:
            out["score"] = np.empty(shape, dtype=np.float64)
            out["ninfo"] = np.empty(shape, dtype=np.int64)
            if likelihoods:
                out["lik"] = np.empty(shape, dtype=np.float64)
                out["lrt"] = np.empty(shape, dtype=np.float64)
        _lib.check_group(self.lib.snpm_group_gather_scores(self.h, ps, pn, m, n_acc, int(in_ld), int(bool(truncate)),
                                                           ptr(out.get("score")), ptr(out.get("ninfo")), ptr(out.get("lik")),
                                                           ptr(out.get("lrt"))), self.h)
        return out

    def gathered_ptrs(self, member=0):
        ds, dn = C.c_void_p(), C.c_void_p()
        _lib.check_group(self.lib.snpm_group_gathered_ptrs(self.h, int(member), C.byref(ds), C.byref(dn)), self.h)
        return ds.value, dn.value

    def free(self):
        if self.h:
            for c in self.contexts:
                if self._owns_contexts:
                    c.close()           # frees the member's panels / queries / carries; the group destroys the context itself
            self.lib.snpm_group_free(self.h)
            self.h = None
            try:
                atexit.unregister(self._atexit)
            except Exception:
                pass

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _on_members(fns):
    """run one callable per group member, each on its own host thread (a context is used by one thread at a time; ctypes
    releases the GIL, so the members' uploads and scoring calls proceed side by side)"""
    if len(fns) == 1:
        return [fns[0]()]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(fns)) as pool:
        futures = [pool.submit(f) for f in fns]
        return [f.result() for f in futures]


class GroupPanel(object):
    """A DB whose accession columns are spread over the GPUs of a ``Group`` driven by this process: member i holds
    columns [a0_i, a1_i) of every SNP row as its own panel (``Panel`` or ``StreamedPanel``).  ``query`` / ``run`` have
    the signatures of ``Panel`` / ``Query`` and return full-length results."""

    def __init__(self, group, members, n_acc):
        assert group.rank0 == 0 and group.world == group.n_local == len(members), "GroupPanel: one process drives the whole group"
        self.group, self.members, self.n_acc = group, members, int(n_acc)
        self.bounds = group.local_shards(n_acc)
        assert all(m.n_acc == a1 - a0 for m, (a0, a1) in zip(members, self.bounds))
        self.n_snp = members[0].n_snp
        self.packed = members[0].packed
        self.ctx = members[0].ctx

    @staticmethod
    def usable_members(n_acc, n_devices):
        """how many members a DB of n_acc accessions can feed (every member needs at least one accession quad)"""
        n = max(1, min(int(n_devices), (int(n_acc) + 3) // 4))
        while n > 1 and (n - 1) * (((n_acc + n - 1) // n + 3) // 4 * 4) >= n_acc:
            n -= 1                      # the last shard would be empty
        return n

    @classmethod
    def build(cls, group, n_acc, make_member):
        """``make_member(ctx, a0, a1)`` -> the member's panel of columns [a0, a1); members are built side by side"""
        bounds = group.local_shards(n_acc)
        assert all(a1 > a0 for a0, a1 in bounds), "more GPUs than accession quads: use GroupPanel.usable_members"
        members = _on_members([(lambda c=c, b=b: make_member(c, b[0], b[1])) for c, b in zip(group.contexts, bounds)])
        return cls(group, members, n_acc)

    @classmethod
    def from_host(cls, group, snps, packed=False):
        return cls.build(group, snps.shape[1], lambda ctx, a0, a1: Panel.from_host(ctx, snps, packed=packed, cols=(a0, a1)))

    def query(self, row_idx, wei, row0=0):
        return GroupQuery(self, row_idx, wei, row0)

    def segregating_rows(self, cols):
        """Genotype.identify_segregating_snps over accessions that live on different GPUs: every member scans the listed
        accessions it holds (local mask + first informative call per row); a row segregates when some member saw two
        different calls or two members saw different ones"""
        cols = np.asarray(cols)
        parts = _on_members([(lambda m=m, b=b: m.segregating_first(cols[(cols >= b[0]) & (cols < b[1])] - b[0]))
                             for m, b in zip(self.members, self.bounds)])
        masks = np.stack([p[0] for p in parts])
        firsts = np.stack([p[1] for p in parts])
        seen = firsts != 0xFF
        lo = np.where(seen, firsts, 255).min(axis=0)
        hi = np.where(seen, firsts, 0).max(axis=0)
        return (masks.any(axis=0) | (seen.any(axis=0) & (lo != hi))).astype(np.uint8)

    def score_batch(self, samples, chunk=1000, skip_hets=False, mode=MODE_EXACT, likelihoods=True, device=None, table=None):
        """``score_batch`` with the accession axis spread over the members: every member scores all samples against its
        columns; the likelihood rows need the minimum over all accessions and are taken on the joined arrays"""
        assert device is None, "device-resident batch inputs belong to one GPU"
        parts = _on_members([(lambda m=m: score_batch(m, samples, chunk, skip_hets, mode, False, None, table)) for m in self.members])
        out = {"score": np.concatenate([p["score"] for p in parts], axis=1),
               "ninfo": np.concatenate([p["ninfo"] for p in parts], axis=1),
               "pairs_reeval": sum(p["pairs_reeval"] for p in parts),
               "strict_fallback": any(p["strict_fallback"] for p in parts)}
        if likelihoods:
            out["lik"], out["lrt"] = self.ctx.likelihood(out["score"], out["ninfo"], truncate=True)
        return out

    def free(self):
        for m in self.members:
            m.free()

    @property
    def h(self):
        """not None while the members' panels are alive (the test ``Genotype.panel`` uses to decide whether to rebuild)"""
        return self.members[0].h


class GroupQuery(object):
    """``Query`` against a ``GroupPanel``: the sample's rows and weights are replicated on every member, every member
    scores its accession shard, one all-gather (RCCL) brings the per-accession results together."""

    def __init__(self, gpanel, row_idx, wei, row0=0):
        self.panel = gpanel
        self.parts = _on_members([(lambda m=m: m.query(row_idx, wei, row0=row0)) for m in gpanel.members])
        self.n = self.parts[0].n
        self._wei = wei

    def run(self, chunk=1000, skip_hets=False, mode=MODE_EXACT, return_info=False):
        gp = self.panel
        ptrs = _on_members([(lambda q=q: q.run_device(chunk, skip_hets, mode)) for q in self.parts])
        out = gp.group.gather([p[0] for p in ptrs], [p[1] for p in ptrs], gp.n_acc)
        if return_info:
            n_re = sum(q.last_reeval() for q in self.parts) if mode == MODE_EXACT else 0
            return out["score"], out["ninfo"], {"n_strict_reeval": int(n_re), "members": len(self.parts),
                                                "transport": gp.group.transport}
        return out["score"], out["ninfo"]

    def run_windows(self, win_off, skip_hets=False, totals=True, fast=False):
        """per-window rows of every member side by side (host arrays: the window table is built on the host), totals
        through the all-gather"""
        res = _on_members([(lambda q=q: q.run_windows(win_off, skip_hets, totals=totals, fast=fast)) for q in self.parts])
        score = np.concatenate([r[0] for r in res], axis=1)
        ninfo = np.concatenate([r[1] for r in res], axis=1)
        tot_s = np.concatenate([r[2] for r in res])
        tot_n = np.concatenate([r[3] for r in res])
        infos = [getattr(q, "last_windows_info", None) for q in self.parts]
        if fast and all(i is not None for i in infos):
            self.last_windows_info = {"pairs_reeval": sum(i["pairs_reeval"] for i in infos),
                                      "totals_reeval": sum(i["totals_reeval"] for i in infos),
                                      "strict_fallback": any(i["strict_fallback"] for i in infos)}
        return score, ninfo, tot_s, tot_n

    def gather_columns(self, acc_idx):
        """calls of the accessions ``acc_idx`` (global indices, on whichever member holds them) at the matched rows"""
        acc_idx = np.asarray(acc_idx)
        out = np.full((len(acc_idx), self.n), 0xFF, dtype=np.uint8)
        for q, (a0, a1) in zip(self.parts, self.panel.bounds):
            mine = np.flatnonzero((acc_idx >= a0) & (acc_idx < a1))
            if len(mine):
                out[mine] = q.gather_columns(acc_idx[mine] - a0)
        return out

    def f1_pairs(self, acc_idx):
        """the in-silico crosses need the listed columns side by side: they are read where they live and crossed on a
        small panel of member 0 (core/csmatch.py:115-125)"""
        acc_idx = np.asarray(acc_idx)
        codes = self.gather_columns(acc_idx)
        ctx = self.panel.members[0].ctx
        small = Panel.from_host(ctx, np.ascontiguousarray(codes.T).view(np.int8))
        q = Query(small, None, self._wei)
        try:
            return q.f1_pairs(np.arange(len(acc_idx)))
        finally:
            q.free()
            small.free()

    def free(self):
        for q in self.parts:
            q.free()


# ----------------------------------------------------------------------------------------------------------
# DBs larger than the HBM budget: the reference streams any size through g.g.snps[idx, :] (core/snpmatch.py:218-225,
# pygwas/genotype.py:548-550).  Here two half-buffers alternate: while the matched rows of piece k are scored, the host
# threads read piece k + 1 from the file and the copy stream brings it in.
class StreamedPanel(object):
    """Columns ``cols`` of a DB (``RowStore``) that does not fit the HBM budget.  ``query`` has ``Panel.query``'s signature; a
    run walks the sample's matched rows in pieces that fit one half-buffer.  The pass is bound by the host link (PCIe
    ~50 GB/s against 5-6 TB/s of HBM), so every piece is scored in the reference's summation order (k_strict4): the fp64
    totals carry the reference's bits after ONE pass over the file, no certificate and no second pass."""

    def __init__(self, ctx, store, cols=None, packed=False, budget_bytes=None):
        self.ctx, self.store = ctx, store
        self.cols = (0, store.n_acc) if cols is None else (int(cols[0]), int(cols[1]))
        self.n_snp, self.n_acc, self.packed = store.n_snp, self.cols[1] - self.cols[0], bool(packed)
        pitch = ctx.row_pitch(self.n_acc, packed)
        if budget_bytes is None:
            budget_bytes = int(0.85 * ctx.mem_info()[0])
        self.rows_cap = int(budget_bytes // 2 // pitch) - 32             # the panel keeps 32 prefetch rows of its own
        assert self.rows_cap >= 1, "HBM budget too small for a single row of this DB"
        self.rows_cap = min(self.rows_cap, max(self.n_snp, 1))
        self.halves = [Panel(ctx, self.rows_cap, self.n_acc, packed=packed, n_acc_total=store.n_acc) for _ in range(2)]
        ctx._children.add(self)
        self._pinned = {}
        self.loads = 0              # pieces loaded so far (tests / timing)

    @property
    def h(self):
        return self.halves[0].h if self.halves else None

    def query(self, row_idx, wei, row0=0):
        return StreamedQuery(self, row_idx, wei, row0)

    def _load(self, which, rows):
        self.store.load(self.halves[which], self.cols, rows, 0)
        self.loads += 1

    def _pieces_of_all_rows(self):
        return [(r, min(r + self.rows_cap, self.n_snp)) for r in range(0, self.n_snp, self.rows_cap)]

    def segregating_first(self, cols):
        """(mask, first) over ALL DB rows (--refine scans the whole DB, core/snp_genotype.py:188-211): piece by piece"""
        masks, firsts = [], []
        for k, (r0, r1) in enumerate(self._pieces_of_all_rows()):
            self._load(k % 2, (r0, r1 - r0))
            m, f = self.halves[k % 2].segregating_first(cols)
            masks.append(m[:r1 - r0])
            firsts.append(f[:r1 - r0])
        return np.concatenate(masks), np.concatenate(firsts)

    def segregating_rows(self, cols):
        out = []
        for k, (r0, r1) in enumerate(self._pieces_of_all_rows()):
            self._load(k % 2, (r0, r1 - r0))
            out.append(self.halves[k % 2].segregating_rows(cols)[:r1 - r0])
        return np.concatenate(out)

    def pinned(self, key, shape, dtype):
        """grow-only pinned host arrays for results that arrive while the next piece is loaded"""
        need = int(np.prod(shape))
        have = self._pinned.get(key)
        if have is None or have.size < need:
            have = self._pinned[key] = self.ctx.pinned_empty((need,), dtype)
        return have[:need].reshape(shape)

    def free(self):
        for p in self.halves:
            p.free()
        self.halves = []
        self._pinned = {}


class StreamedQuery(object):
    """``Query`` against a ``StreamedPanel``: same calls, same results (reference order, fp64 bit for bit)."""

    def __init__(self, spanel, row_idx, wei, row0=0):
        wei = np.asarray(wei)
        assert wei.ndim == 2 and wei.shape[1] == 3, "SNP weights should be a np.array with  shape == n,3"
        self.panel, self.wei = spanel, np.ascontiguousarray(wei, dtype=np.float64)
        self.n = self.wei.shape[0]
        if row_idx is None:
            self.rows = np.arange(int(row0), int(row0) + self.n, dtype=np.int64)
        else:
            self.rows = np.ascontiguousarray(row_idx, dtype=np.int64)
            assert self.rows.shape == (self.n,), "please provide same number of positions for both sample and db"
        assert self.n == 0 or (self.rows.min() >= 0 and self.rows.max() < spanel.n_snp), "row index outside the panel"

    def _walk(self, bounds, score_piece):
        """load the matched rows [i0, i1) of every piece into alternating half-buffers and hand (half, i0, i1, k) to
        ``score_piece``, which only ENQUEUES device work: the next piece is read and copied in while it runs"""
        sp = self.panel
        if not bounds:
            return
        import os
        import time
        trace = [] if os.environ.get("SNPM_STREAM_TRACE") else None
        t0 = time.perf_counter()
        sp._load(0, self.rows[bounds[0][0]:bounds[0][1]])
        if trace is not None:
            trace.append(("load", 0, time.perf_counter() - t0))
        for k, (i0, i1) in enumerate(bounds):
            t0 = time.perf_counter()
            score_piece(sp.halves[k % 2], i0, i1, k)
            t1 = time.perf_counter()
            if k + 1 < len(bounds):
                j0, j1 = bounds[k + 1]
                sp._load((k + 1) % 2, self.rows[j0:j1])
            if trace is not None:
                trace.append(("enqueue", k, t1 - t0))
                trace.append(("load", k + 1, time.perf_counter() - t1))
        if trace is not None:
            import sys
            sys.stderr.write("stream trace: " + ", ".join("%s[%d] %.3f s" % t for t in trace) + "\n")

    def _run_carry(self, chunk, skip_hets, mode):
        sp = self.panel
        chunk = int(chunk)
        per = sp.rows_cap // chunk * chunk
        assert per >= chunk, "HBM budget too small for one %d-row chunk of this DB" % chunk
        bounds = [(i, min(i + per, self.n)) for i in range(0, self.n, per)]     # pieces of the MATCHED list, cut at chunk boundaries
        carry = Carry(sp.ctx, sp.n_acc)
        m = MODE_FAST if mode == MODE_FAST else MODE_STRICT
        live = []

        def score_piece(half, i0, i1, k):
            q = Query(half, None, self.wei[i0:i1])
            after = sum(-(-(b1 - b0) // chunk) for b0, b1 in bounds[k + 1:])
            q.run_carry(carry, chunk, skip_hets, m, after)
            live.append(q)
            if len(live) > 2:                   # the query of piece k - 2 has long finished
                live.pop(0).free()

        self._walk(bounds, score_piece)
        carry.finish(want_results=False)            # waits for the last piece
        for q in live:
            q.free()
        return carry, len(bounds)

    def run(self, chunk=1000, skip_hets=False, mode=MODE_EXACT, return_info=False):
        carry, n_pieces = self._run_carry(chunk, skip_hets, mode)
        score, ninfo, _ = carry.finish()
        carry.free()
        if return_info:
            return score, ninfo, {"n_strict_reeval": 0, "all_integer_weights": False, "reeval_path": 0, "pieces": n_pieces}
        return score, ninfo

    def run_device(self, chunk=1000, skip_hets=False, mode=MODE_EXACT):
        """results left on the device (raw pointers, valid until the next run / free): what a GroupQuery gathers"""
        if getattr(self, "_carry", None) is not None:
            self._carry.free()
        self._carry, _ = self._run_carry(chunk, skip_hets, mode)
        return self._carry.device_ptrs()

    def last_reeval(self):
        return 0

    def _window_pieces(self, win_off):
        sp = self.panel
        pieces, w0 = [], 0
        n_win = len(win_off) - 1
        while w0 < n_win:
            w1 = w0 + 1
            assert win_off[w1] - win_off[w0] <= sp.rows_cap, "HBM budget too small for the SNPs of one window"
            while w1 < n_win and win_off[w1 + 1] - win_off[w0] <= sp.rows_cap:
                w1 += 1
            pieces.append((w0, w1))
            w0 = w1
        return pieces

    def run_windows(self, win_off, skip_hets=False, totals=True, fast=False):
        """per-window matchGTsAccs over a streamed DB: pieces hold whole windows, the totals' chain continues in a carry"""
        sp = self.panel
        ctx = sp.ctx
        win_off = np.ascontiguousarray(win_off, dtype=np.int64)
        n_win = len(win_off) - 1
        p_score = sp.pinned("w_score", (max(n_win, 1), sp.n_acc), np.float64)
        p_ninfo = sp.pinned("w_ninfo", (max(n_win, 1), sp.n_acc), np.int64)
        carry = Carry(ctx, sp.n_acc)
        pieces = self._window_pieces(win_off)
        live = []

        def score_piece(half, i0, i1, k):
            w0, w1 = pieces[k]
            q = Query(half, None, self.wei[i0:i1])
            off = np.ascontiguousarray(win_off[w0:w1 + 1] - i0)
            check(ctx.lib.snpm_query_run_windows_carry(q.h, ptr(off), w1 - w0, int(bool(skip_hets)), ptr(p_score[w0:w1]),
                                                       ptr(p_ninfo[w0:w1]), carry.h), ctx.h)
            live.append(q)
            if len(live) > 2:
                live.pop(0).free()

        self._walk([(int(win_off[w0]), int(win_off[w1])) for w0, w1 in pieces], score_piece)
        tot_s, tot_n, _ = carry.finish()            # waits for the device: the pinned rows are complete
        for q in live:
            q.free()
        carry.free()
        return np.array(p_score[:n_win]), np.array(p_ninfo[:n_win]), tot_s, tot_n

    def gather_columns(self, acc_idx):
        sp = self.panel
        per = sp.rows_cap
        out = []

        def piece(half, i0, i1, k):
            q = Query(half, None, self.wei[i0:i1])
            out.append(q.gather_columns(acc_idx))
            q.free()

        self._walk([(i, min(i + per, self.n)) for i in range(0, self.n, per)], piece)
        return np.concatenate(out, axis=1) if out else np.zeros((len(acc_idx), 0), dtype=np.uint8)

    def f1_pairs(self, acc_idx):
        """in-silico crosses: the listed columns at the matched rows are read piece by piece, then crossed on a small panel"""
        acc_idx = np.asarray(acc_idx)
        codes = self.gather_columns(acc_idx)
        small = Panel.from_host(self.panel.ctx, np.ascontiguousarray(codes.T).view(np.int8))
        q = Query(small, None, self.wei)
        try:
            return q.f1_pairs(np.arange(len(acc_idx)))
        finally:
            q.free()
            small.free()

    def free(self):
        if getattr(self, "_carry", None) is not None:
            self._carry.free()
            self._carry = None
