"""Host-side mirror of the reference's stage interface (src/main.h:1-8, call order src/main.c:83-149)
over the C ABI of libdebwt_hip.so.  Same stage names and order; state lives in a context object instead
of globals and temp files; errors raise DebwtError instead of exit(1)."""
import ctypes

import numpy as np

from . import _lib

ARR_SORTED_KEYS, ARR_DISTINCT_KEYS, ARR_RED, ARR_SP_SYMBOLS, ARR_BLUE, ARR_BLUE_BOUND, ARR_CASE3_BOUND, \
    ARR_ROW_SYMBOLS = range(1, 9)
DUMP_KMERINFO, DUMP_BLOCKS, DUMP_SP = 1, 2, 3
_ARR_DTYPE = {ARR_SP_SYMBOLS: np.uint8, ARR_ROW_SYMBOLS: np.uint8}


class DebwtError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = _lib.lib().debwt_strerror(code).decode()
        super().__init__(f"{msg} ({code})" + (f": {detail}" if detail else ""))


def _p64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def pack_records(records):
    """2-bit packed text in the reference layout (src/collect#$.c:61-90): base j at bit
    2*(31-(j&31)) of word j>>5, 'T' at every separator, 32 'T' of padding.  records: list of uint8
    code arrays (A0 C1 G2 T3).  Returns (words, n, sep)."""
    lens = np.array([len(r) for r in records], dtype=np.uint64)
    if (lens <= 32).any():
        raise ValueError("every record must be longer than 32 bases (src/collect#$.c:41-45)")
    n = int(lens.sum()) + len(records)
    total = n + 32
    nwords = (total + 31) // 32 + 1
    sym = np.full(nwords * 32, 3, dtype=np.uint8)
    sym[total:] = 0
    sep = np.empty(len(records), dtype=np.uint64)
    o = 0
    for i, r in enumerate(records):
        r = np.asarray(r, dtype=np.uint8)
        if r.size and r.max() > 3:
            raise ValueError("codes must be 0..3")
        sym[o:o + len(r)] = r
        o += len(r)
        sep[i] = o
        o += 1
    q = sym.reshape(-1, 4)
    b = (q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]
    words = np.ascontiguousarray(b).view(">u8").astype(np.uint64)
    return words, n, sep


class DeBWT:
    """One context = one GPU.  Typical use:
        d = DeBWT(k=32); d.load_records(records); d.build(); words, hash_rows, dollar_row = d.fetch()
    or stage by stage: kmer_sort_rle(), classify(), sp_generate(), blue_sort(), bwt_assemble()."""

    def __init__(self, k=32, device=0, sort_algo=0, tune=0):
        self._L = _lib.lib()
        cfg = _lib.DebwtConfig(k=k, device=device, sort_algo=sort_algo, reserved=tune)
        h = ctypes.c_void_p()
        rc = self._L.debwt_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc:
            raise DebwtError(rc)
        self._h = h
        self.k = k
        self.n = 0
        self.nrec = 0
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.debwt_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc:
            raise DebwtError(rc, self._L.debwt_last_error(self._h).decode())

    # -- loading ------------------------------------------------------------------------------------
    def load_packed(self, words, n, sep):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        sep = np.ascontiguousarray(sep, dtype=np.uint64)
        self._keep = (words, sep)       # the library reads the host text during a run
        self._chk(self._L.debwt_load_text(self._h, _p64(words), n, _p64(sep), len(sep)))
        self.n, self.nrec = n, len(sep)

    def load_records(self, records):
        words, n, sep = pack_records(records)
        self.load_packed(words, n, sep)

    def load_ascii(self, records):
        recs = [r.encode() if isinstance(r, str) else bytes(r) for r in records]
        lens = np.array([len(r) for r in recs], dtype=np.uint64)
        self._chk(self._L.debwt_load_ascii(self._h, b"".join(recs), _p64(lens), len(recs)))
        self.n, self.nrec = int(lens.sum()) + len(recs), len(recs)

    def load_fasta(self, path, threads=8, iupac_seed=None):
        """FASTA (plain or gzip) parsed and packed by `threads` host threads, then loaded.  iupac_seed: replace N and
        the other ambiguity letters by pseudo-random bases of their sets (deterministic in seed and position)."""
        if iupac_seed is None:
            self._chk(self._L.debwt_load_fasta(self._h, str(path).encode(), int(threads)))
        else:
            self._chk(self._L.debwt_load_fasta_opts(self._h, str(path).encode(), int(threads), FASTA_IUPAC_RANDOM, int(iupac_seed)))
        st = self.stats()
        self.n, self.nrec = st["n"], st["nrec"]

    def reserve(self, n, nrec, branching=0.0, one_shot=False, compact=False):
        """Allocate the workspace of a text of up to n symbols in nrec records ahead of the load (debwt_reserve): call it
        on a thread of its own while the input is still being read -- ctypes releases the GIL for the call."""
        self._chk(self._L.debwt_reserve(self._h, int(n), int(nrec), float(branching), (1 if one_shot else 0) | (2 if compact else 0)))

    def set_range_cap(self, max_instances):
        """Largest number of node instances sorted in one go; larger texts are built in k-mer-prefix ranges."""
        self._chk(self._L.debwt_set_range_cap(self._h, int(max_instances)))

    # -- stages (src/main.c:83-149) -------------------------------------------------------------------
    def kmer_sort_rle(self):
        self._chk(self._L.debwt_kmer_sort_rle(self._h))

    def classify(self):
        self._chk(self._L.debwt_classify(self._h))

    def sp_generate(self):
        self._chk(self._L.debwt_sp_generate(self._h))

    def blue_sort(self):
        self._chk(self._L.debwt_blue_sort(self._h))

    def bwt_assemble(self):
        self._chk(self._L.debwt_bwt_assemble(self._h))

    def build(self):
        self._chk(self._L.debwt_build(self._h))

    # -- results --------------------------------------------------------------------------------------
    def fetch(self):
        words = np.empty((self.n + 31) // 32, dtype=np.uint64)
        hrows = np.empty(max(self.nrec - 1, 1), dtype=np.uint64)
        drow = np.empty(1, dtype=np.uint64)
        self._chk(self._L.debwt_fetch_bwt(self._h, _p64(words), _p64(hrows), _p64(drow)))
        return words, hrows[:self.nrec - 1], int(drow[0])

    def fetch_into(self, words, hrows, drow):
        """fetch() into caller-owned uint64 arrays (e.g. page-locked ones): ceil(n/32), nrec-1 (>= 1), 1 words."""
        self._chk(self._L.debwt_fetch_bwt(self._h, _p64(words), _p64(hrows), _p64(drow)))

    def build_into(self, words, hrows, drow):
        """build() + fetch_into() with the copy of finished row ranges hidden behind the blue sort of the following ones
        (debwt_build_to_host); page-locked arrays for the overlap."""
        self._chk(self._L.debwt_build_to_host(self._h, _p64(words), _p64(hrows), _p64(drow)))

    def fetch_small(self):
        """(None, hash_rows, dollar_row): the row lists only, the BWT words stay in HBM."""
        hrows = np.empty(max(self.nrec - 1, 1), dtype=np.uint64)
        drow = np.empty(1, dtype=np.uint64)
        self._chk(self._L.debwt_fetch_rows(self._h, _p64(hrows), _p64(drow)))
        return None, hrows[:self.nrec - 1], int(drow[0])

    def bwt_census(self):
        """Rows of the result per 2-bit code (computed on the device)."""
        c = np.zeros(4, dtype=np.uint64)
        self._chk(self._L.debwt_bwt_census(self._h, _p64(c)))
        return c

    def verify_device(self, d_words=None, hash_rows=None, dollar_row=0, segments=0):
        """Inverse BWT on the device against the loaded text (debwt_verify_device).  Default: the context's own result;
        otherwise d_words = device address of packed rows, hash_rows / dollar_row their row lists."""
        rep = _lib.DebwtVerifyReport()
        hp = None
        if d_words is not None and hash_rows is not None and len(hash_rows):
            hash_rows = np.ascontiguousarray(hash_rows, dtype=np.uint64)
            hp = _p64(hash_rows)
        self._chk(self._L.debwt_verify_device(self._h, ctypes.c_void_p(d_words) if d_words else None, hp, int(dollar_row),
                                              int(segments), ctypes.byref(rep)))
        r = rep.as_dict()
        return {"inverse_bwt_ok": bool(r["ok"]), "inverse_bwt": {k: (round(v, 2) if isinstance(v, float) else v)
                                                                  for k, v in r.items() if k != "ok"}}

    def fm_index(self, sa_sample=32, rows=None):
        """FM-index of the rows (debwt_fm_create): the context's own result, or host rows = (words, hash_rows, dollar_row)
        as fetch() returns them / OUT, OUT.#, OUT.$ hold them.  Rows that are not the BWT of the loaded text raise.  The
        index outlives this context."""
        h = ctypes.c_void_p()
        if rows is None:
            rc = self._L.debwt_fm_create(self._h, None, None, 0, int(sa_sample), ctypes.byref(h))
        else:
            words, hrows, drow = rows
            words = np.ascontiguousarray(words, dtype=np.uint64)
            hrows = np.ascontiguousarray(hrows, dtype=np.uint64)
            rc = self._L.debwt_fm_create(self._h, _p64(words), _p64(hrows) if len(hrows) else None, int(drow),
                                         int(sa_sample), ctypes.byref(h))
        self._chk(rc)
        return FMIndex(h)

    def special_compare(self):
        """Special-region tables of the loaded text, device module against host module: mismatching elements of
        (suffix order, keys, BWT symbols, special branches, head nodes, tail nodes) -- all zero when they agree."""
        mm = np.zeros(6, dtype=np.uint64)
        self._chk(self._L.debwt_special_compare(self._h, _p64(mm)))
        return [int(x) for x in mm]

    def stats(self):
        st = _lib.DebwtStats()
        self._chk(self._L.debwt_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def fetch_array(self, which):
        cnt = ctypes.c_uint64()
        self._chk(self._L.debwt_fetch_array(self._h, which, None, 0, ctypes.byref(cnt)))
        out = np.empty(max(cnt.value, 1), dtype=_ARR_DTYPE.get(which, np.uint64))
        self._chk(self._L.debwt_fetch_array(self._h, which, out.ctypes.data_as(ctypes.c_void_p), cnt.value,
                                            ctypes.byref(cnt)))
        return out[:cnt.value]

    def dump_reference_files(self, directory, stage):
        """Intermediates of the stage just run as files in the reference's byte formats (debwt_dump_reference_files):
        stage DUMP_KMERINFO (kmerInfo), DUMP_BLOCKS after classify() (redSeq, redPoint, blueBound, case3bound),
        DUMP_SP after sp_generate() (spCode, spSpecialIndex, blueTable)."""
        self._chk(self._L.debwt_dump_reference_files(self._h, str(directory).encode(), int(stage)))

    def kmer_count_sorted(self):
        """(kmers left-aligned, counts): the contents of the reference's kmerInfo (src/mySort.c:193-195)."""
        d = ctypes.c_uint64()
        self._chk(self._L.debwt_kmer_count_sorted(self._h, None, None, 0, ctypes.byref(d)))
        km = np.empty(max(d.value, 1), dtype=np.uint64)
        ct = np.empty(max(d.value, 1), dtype=np.uint64)
        self._chk(self._L.debwt_kmer_count_sorted(self._h, _p64(km), _p64(ct), d.value, ctypes.byref(d)))
        return km[:d.value], ct[:d.value]

    def radix_sort_device(self, keys_ptr, tmp_ptr, count, key_bits=64, want_ms=False, key_lo=0, key_hi=0):
        """Sort `count` u64 keys resident in HBM (raw device pointers, e.g. torch tensor .data_ptr()).
        key_lo, key_hi: bounds the caller vouches for, every key in [key_lo, key_hi) (key_hi = 0: no upper bound)."""
        ms = ctypes.c_float()
        self._chk(self._L.debwt_radix_sort_u64_range(self._h, ctypes.c_void_p(keys_ptr), ctypes.c_void_p(tmp_ptr), count,
                                                     key_bits, int(key_lo), int(key_hi), ctypes.byref(ms) if want_ms else None))
        return ms.value

    def radix_bucket_passes(self):
        """Sorts of this process whose lowest prefix digit was split bucket by bucket in LDS (debwt_radix_bucket_passes;
        DEBWT_BUCKET_PASS=0 / 1 in the environment switch that form off / on everywhere)."""
        return int(self._L.debwt_radix_bucket_passes())

    def bwt_device_ptr(self):
        p = ctypes.c_void_p()
        self._chk(self._L.debwt_bwt_device_ptr(self._h, ctypes.byref(p)))
        return p.value


def _patterns(patterns):
    """(concatenated bytes, offsets) of one str/bytes pattern or a sequence of them"""
    if isinstance(patterns, tuple) and len(patterns) == 2 and isinstance(patterns[1], np.ndarray):
        return patterns                                       # made by an earlier _patterns()
    if isinstance(patterns, (str, bytes, bytearray)):
        patterns = [patterns]
    enc = [p.encode() if isinstance(p, str) else bytes(p) for p in patterns]
    offs = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        np.cumsum([len(p) for p in enc], out=offs[1:])
    return b"".join(enc), offs


class FMIndex:
    """FM-index over built rows on one GPU (debwt_fm_*): count and locate exact patterns of A/C/G/T (either case).  Made
    by DeBWT.fm_index() from a loaded text, or by FMIndex.open() from saved rows and samples alone.  Positions are global
    text positions (records joined by one separator each); resolve() turns them into (record, offset)."""

    def __init__(self, handle):
        self._L = _lib.lib()
        self._h = handle
        info = self.info()
        self.n, self.nrec, self.sa_sample = info["n"], info["nrec"], info["sa_sample"]
        starts = np.empty(max(self.nrec, 1), dtype=np.uint64)
        self._chk(self._L.debwt_fm_record_starts(self._h, _p64(starts), len(starts)))
        self._starts = starts[:self.nrec]

    @classmethod
    def open(cls, words, n, hash_rows, dollar_row, samples, sa_sample=32, device=0):
        """The index from rows (OUT), the '#' rows (OUT.#), the '$' row (OUT.$) and samples() of an index of them."""
        L = _lib.lib()
        words = np.ascontiguousarray(words, dtype=np.uint64)
        hrows = np.ascontiguousarray(hash_rows, dtype=np.uint64)
        samples = np.ascontiguousarray(samples, dtype=np.uint64)
        if len(words) < (int(n) + 31) // 32 or len(samples) < (int(n) + sa_sample - 1) // sa_sample:
            raise ValueError("rows or samples shorter than n asks for")
        h = ctypes.c_void_p()
        rc = L.debwt_fm_open(int(device), _p64(words), int(n), _p64(hrows) if len(hrows) else None, len(hrows) + 1,
                             int(dollar_row), _p64(samples), int(sa_sample), ctypes.byref(h))
        if rc:
            raise DebwtError(rc)
        return cls(h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.debwt_fm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc:
            raise DebwtError(rc, self._L.debwt_fm_last_error(self._h).decode())

    def info(self):
        inf = _lib.DebwtFmInfo()
        self._chk(self._L.debwt_fm_info_get(self._h, ctypes.byref(inf)))
        return inf.as_dict()

    def samples(self):
        """The sampled suffix array: position of row i * sa_sample, ceil(n / sa_sample) words (save it for open())."""
        out = np.empty(self.info()["samples"], dtype=np.uint64)
        self._chk(self._L.debwt_fm_samples(self._h, _p64(out), len(out)))
        return out

    def record_starts(self):
        return self._starts.copy()

    def ranges(self, patterns):
        """(npat, 2) uint64 row intervals [lo, hi) of the suffixes that start with each pattern."""
        buf, offs = _patterns(patterns)
        out = np.zeros((len(offs) - 1, 2), dtype=np.uint64)
        if len(out):
            self._chk(self._L.debwt_fm_count(self._h, buf, _p64(offs), len(out), _p64(out)))
        return out

    def count(self, patterns):
        """Occurrences of each pattern (np.uint64); empty patterns and any with a letter outside ACGTacgt: 0."""
        r = self.ranges(patterns)
        return r[:, 1] - r[:, 0]

    def locate(self, patterns, max_per_pattern=None):
        """Global text positions of each pattern's occurrences (the first max_per_pattern rows when capped), one uint64
        array per pattern, in row (suffix) order."""
        r = np.ascontiguousarray(self.ranges(patterns))
        npat = len(r)
        offs = np.zeros(npat + 1, dtype=np.uint64)
        cnt = r[:, 1] - r[:, 0]
        if max_per_pattern is not None:
            cnt = np.minimum(cnt, np.uint64(max_per_pattern))
        total = int(cnt.sum())
        pos = np.empty(max(total, 1), dtype=np.uint64)
        if npat:
            self._chk(self._L.debwt_fm_locate(self._h, _p64(r), npat, int(max_per_pattern or 0), _p64(offs), _p64(pos),
                                              len(pos)))
        return [pos[int(offs[i]):int(offs[i + 1])] for i in range(npat)]

    def resolve(self, positions):
        """(record, offset) arrays of global text positions."""
        p = np.asarray(positions, dtype=np.uint64)
        rec = np.searchsorted(self._starts, p, side="right").astype(np.int64) - 1
        return rec, p - self._starts[rec]

    def search(self, patterns, mismatches=1, strands="forward", best=False):
        """Hits with up to `mismatches` (0..4) substitutions among A/C/G/T (debwt_fm_search): one hit per distinct text
        string, as its row interval, mismatch count and strand (0 forward, 1 reverse complement).  strands: "forward" or
        "both"; best: only each pattern's hits of the smallest mismatch count.  A character outside ACGTacgt matches no
        base.  Returns a SearchResult."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        flags = (SEARCH_BOTH_STRANDS if strands == "both" else 0) | (SEARCH_BEST_ONLY if best else 0)
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        hoff = np.zeros(npat + 1, dtype=np.uint64)
        cap = 4 * npat + 16                                   # first estimate; grown to the exact count on DEBWT_ERANGE
        while True:
            ranges = np.zeros((cap, 2), dtype=np.uint64)
            info = np.zeros(cap, dtype=np.uint32)
            rc = self._L.debwt_fm_search(self._h, buf, _p64(offs), npat, int(mismatches), flags, _p64(hoff), _p64(ranges),
                                         info.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap)
            if rc == -5 and int(hoff[npat]) > cap:
                cap = int(hoff[npat])
                continue
            self._chk(rc)
            break
        h = int(hoff[npat])
        return SearchResult(self, hoff, ranges[:h].copy(), (info[:h] & 0xFF).astype(np.uint8),
                            ((info[:h] >> 8) & 1).astype(np.uint8))

    def search_stats(self):
        """What the last search did (debwt_fm_search_stats_get): items per level, rank steps and lines, kernel ms."""
        st = _lib.DebwtFmSearchStats()
        self._chk(self._L.debwt_fm_search_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def mems(self, patterns, min_len=19, strands="forward"):
        """Maximal exact matches of each pattern of at least min_len bases (debwt_fm_mems; 19 is BWA-MEM's -k): spans of
        the pattern that occur inside one record and cannot be extended by one base on either side and still occur.
        strands "both" adds those of the reverse complement (strand 1), with spans in the pattern's own coordinates.
        A character outside ACGTacgt matches nothing.  Returns a MemResult."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        flags = SEARCH_BOTH_STRANDS if strands == "both" else 0
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        moff = np.zeros(npat + 1, dtype=np.uint64)
        cap = 4 * npat + 16                                   # first estimate; grown to the exact count on DEBWT_ERANGE
        while True:
            spans = np.zeros((cap, 2), dtype=np.uint32)
            ranges = np.zeros((cap, 2), dtype=np.uint64)
            st = np.zeros(cap, dtype=np.uint8)
            rc = self._L.debwt_fm_mems(self._h, buf, _p64(offs), npat, int(min_len), flags, _p64(moff),
                                       spans.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _p64(ranges),
                                       st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap)
            if rc == -5 and int(moff[npat]) > cap:
                cap = int(moff[npat])
                continue
            self._chk(rc)
            break
        h = int(moff[npat])
        return MemResult(self, moff, spans[:h].copy(), ranges[:h].copy(), st[:h].copy())

    def mems_stats(self):
        """What the last mems call did (debwt_fm_mems_stats_get): batches, MEMs, rank steps and lines, wave steps, ms."""
        st = _lib.DebwtFmMemsStats()
        self._chk(self._L.debwt_fm_mems_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def overlaps(self, patterns, min_overlap=20, strands="forward", longest=False):
        """Suffix-prefix overlaps (debwt_fm_overlaps): for each pattern every (record, length) with length >= min_overlap
        whose record begins with the pattern's last `length` bases, the pattern's own record and containments included.
        strands "both" adds the overlaps of the reverse complement (strand 1: the record begins with the reverse
        complement of the pattern's FIRST `length` bases).  longest: per (pattern, strand, record) only the largest
        length.  No attached text is needed.  Returns an OverlapResult."""
        return self._overlaps(patterns, strands, longest, lambda buf, offs, npat, flags, *out: self._L.debwt_fm_overlaps(
            self._h, buf, offs, npat, int(min_overlap), flags, *out))

    def _overlaps(self, patterns, strands, longest, call):
        """overlaps() and overlaps_mm(): call(buf, offsets, npat, flags, hit_offsets, hits, capacity) is the bound C call"""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        flags = (SEARCH_BOTH_STRANDS if strands == "both" else 0) | (OVERLAP_LONGEST if longest else 0)
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        hoff = np.zeros(npat + 1, dtype=np.uint64)
        cap = 4 * npat + 16                                   # first estimate; grown to the exact count on DEBWT_ERANGE
        while True:
            hits = np.zeros(cap, dtype=_OVERLAP_DTYPE)
            rc = call(buf, _p64(offs), npat, flags, _p64(hoff), hits.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmOverlap)), cap)
            if rc == -5 and int(hoff[npat]) > cap:
                cap = int(hoff[npat])
                continue
            self._chk(rc)
            break
        return OverlapResult(self, hoff, hits[:int(hoff[npat])].copy())

    def overlaps_stats(self):
        """What the last overlaps call did (debwt_fm_overlaps_stats_get): batches, runs, hits, rank steps and lines, wave
        steps, scratch bytes, ms."""
        st = _lib.DebwtFmOverlapsStats()
        self._chk(self._L.debwt_fm_overlaps_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def overlaps_mm(self, patterns, min_overlap=20, mismatches=1, error_permille=0, strands="forward", longest=False):
        """Suffix-prefix overlaps with substitutions (debwt_fm_overlaps_mm): every (record, length) with length >=
        min_overlap whose first `length` bases differ from the pattern's last `length` in at most `mismatches` (0..4)
        columns and, with error_permille R > 0, in at most R / 1000 of them; a character outside ACGTacgt is a mismatch.
        Patterns hold at most 1024 bytes.  strands and longest as in overlaps(); the order is that of overlaps(), and
        mismatches=0 gives its result.  Returns an OverlapResult whose mismatches() are the counts per hit."""
        return self._overlaps(patterns, strands, longest, lambda buf, offs, npat, flags, *out: self._L.debwt_fm_overlaps_mm(
            self._h, buf, offs, npat, int(min_overlap), int(mismatches), int(error_permille), flags, *out))

    def overlaps_mm_stats(self):
        """What the last overlaps_mm call did (debwt_fm_overlaps_mm_stats_get): batches, launches and re-run launches, runs,
        hits, work items per mismatch level, rank steps and lines, wave steps, scratch bytes, ms."""
        st = _lib.DebwtFmOverlapsMmStats()
        self._chk(self._L.debwt_fm_overlaps_mm_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def kmer_counts(self, patterns, k, strands="forward"):
        """The count of every k-mer along every pattern (debwt_fm_kmer_counts): occurrences inside one record, 0 for a
        k-mer with a character outside ACGTacgt; strands "both" adds the occurrences of the reverse complement (a k-mer
        that is its own reverse complement counts twice).  Counts are uint32, clamped at 2^32 - 1.  A pattern shorter than
        k has no k-mers.  No attached text is needed.  Returns a KmerResult."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        flags = SEARCH_BOTH_STRANDS if strands == "both" else 0
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        k = int(k)
        coff = np.zeros(npat + 1, dtype=np.uint64)
        cap = int(np.maximum(np.diff(offs.astype(np.int64)) - (k - 1), 0).sum()) if k > 0 else 0
        counts = np.zeros(max(cap, 1), dtype=np.uint32)
        self._chk(self._L.debwt_fm_kmer_counts(self._h, buf, _p64(offs), npat, k, flags, _p64(coff),
                                               counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap))
        return KmerResult(coff, counts[:int(coff[npat])])

    def kmer_stats(self):
        """What the last kmer_counts call did (debwt_fm_kmer_stats_get): batches, k-mers, rank steps and lines, wave
        steps, walks started from the prefix table, its q and build time, scratch bytes, ms."""
        st = _lib.DebwtFmKmerStats()
        self._chk(self._L.debwt_fm_kmer_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def spectrum(self, k, strands="both", bins=256):
        """The k-mer spectrum of the indexed collection (debwt_fm_spectrum): every distinct k-mer inside a record is met
        once by a walk over the index; strands "both" counts a k-mer with its reverse complement under the smaller code
        (a k-mer that is its own reverse complement counts twice, as in kmer_counts).  hist[c] is the number of distinct
        k-mers of multiplicity c, the last bin holds bins - 1 and above.  No reads and no attached text are needed.
        Returns a SpectrumResult."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        hist = np.zeros(max(int(bins), 1), dtype=np.uint64)
        tot = _lib.DebwtFmSpectrumTotals()
        self._chk(self._L.debwt_fm_spectrum(self._h, int(k), SEARCH_BOTH_STRANDS if strands == "both" else 0, int(bins),
                                            _p64(hist), ctypes.byref(tot)))
        return SpectrumResult(int(k), strands, hist, int(tot.distinct), int(tot.total), int(tot.overflow_total))

    def kmer_list(self, k, strands="both", min_count=1, max_count=2**32 - 1):
        """The distinct k-mers with min_count <= multiplicity <= max_count (debwt_fm_kmer_list), ascending by code:
        (codes uint64, counts uint32).  A code holds A, C, G, T as 0..3 with the first character in the most significant
        digit (kmer_string turns it back into letters); counts are clamped at 2^32 - 1."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        flags = SEARCH_BOTH_STRANDS if strands == "both" else 0
        n = ctypes.c_uint64(0)
        args = (self._h, int(k), flags, int(min_count), int(max_count))
        rc = self._L.debwt_fm_kmer_list(*args, None, None, 0, ctypes.byref(n))      # the sizing call: ERANGE names the count
        if rc != -5:
            self._chk(rc)
        codes = np.zeros(max(n.value, 1), dtype=np.uint64)
        counts = np.zeros(max(n.value, 1), dtype=np.uint32)
        if n.value:
            self._chk(self._L.debwt_fm_kmer_list(*args, _p64(codes), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                 n.value, ctypes.byref(n)))
        return codes[:n.value], counts[:n.value]

    def spectrum_stats(self):
        """What the last spectrum or kmer_list call did (debwt_fm_spectrum_stats_get): chunks, launches, levels, intervals
        expanded and per depth, leaves, reverse-complement look-ups, rank steps and lines, wave steps, scratch bytes, the
        limit in force, the table's q and ms."""
        st = _lib.DebwtFmSpectrumStats()
        self._chk(self._L.debwt_fm_spectrum_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def esa(self, max_lcp=0, sa=False, da=False):
        """Suffix array, LCP array and record array of the collection on the device (debwt_fm_esa_build, Definition 10):
        lcp[r] is the common prefix of the suffixes of rows r - 1 and r, cut at the first separator of either and stored
        as min(lcp, max_lcp) (max_lcp 0: no cap); sa and da keep the positions and the records of the rows as well.  The
        text is restored first when none is attached.  The arrays stay on the device, counted in info()["device_bytes"],
        until release() or the next esa(), which replaces them.  Returns an EsaResult."""
        flags = (ESA_SA if sa else 0) | (ESA_DA if da else 0)
        self._chk(self._L.debwt_fm_esa_build(self._h, int(max_lcp), flags))
        return EsaResult(self)

    def esa_stats(self):
        """What the last esa() did (debwt_fm_esa_stats_get): walk items, LF steps and wave steps, chunks and the chunk
        length in force (DEBWT_FM_ESA_CHUNK), symbols_compared and plcp_wave_steps of the PLCP kernel, bytes allocated by
        the build and kept, ms per phase and wall ms."""
        st = _lib.DebwtFmEsaStats()
        self._chk(self._L.debwt_fm_esa_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def repeat_stats(self):
        """What the last EsaResult.repeats did (debwt_fm_repeat_stats_get): rows, rows searched, representatives, intervals,
        maximal, supermaximal, capped_intervals, reported, the longest reported length and its row_lo, levels and fanout of
        the hierarchy (DEBWT_FM_REPEAT_FANOUT), tree and scratch bytes, search_steps and wave_steps of the searches, rank
        lines read, ms per phase and wall ms."""
        st = _lib.DebwtFmRepeatStats()
        self._chk(self._L.debwt_fm_repeat_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def cdbg_stats(self):
        """What the last EsaResult.cdbg did (debwt_fm_cdbg_stats_get): nodes, edge_strings, unitigs, circular, links, edges,
        longest_nodes, seq_bytes, jump_rounds, jump_steps and jump_wave_steps of the ranking, rank lines read, scratch
        bytes, ms per phase and wall ms."""
        st = _lib.DebwtFmCdbgStats()
        self._chk(self._L.debwt_fm_cdbg_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def cdbg_both_stats(self):
        """What the last EsaResult.cdbg(k, strands="both") did (debwt_fm_cdbg_both_stats_get): the counting fields of
        cdbg_stats over reported unitigs and canonical nodes, present, mated, hairpins, the ranking's rounds and steps, rank
        lines, mate_steps, edge_keys, scratch bytes, ms per phase and wall ms."""
        st = _lib.DebwtFmCdbgBothStats()
        self._chk(self._L.debwt_fm_cdbg_both_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def records_stats(self):
        """What the last EsaResult.records_build did (debwt_fm_records_stats_get): rows, pairs (rows whose record occurs in
        an earlier row), records_present, sort_passes, levels and fanout of the hierarchy (DEBWT_FM_REPEAT_FANOUT),
        rmq_steps and wave_steps of the range minima, bytes allocated by the build and kept, ms per phase and wall ms."""
        st = _lib.DebwtFmRecordsStats()
        self._chk(self._L.debwt_fm_records_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def correct(self, patterns, k, min_count=3, rounds=4, strands="both"):
        """k-mer read correction on the device (debwt_fm_correct): per read and round, a run of weak k-mers (count below
        min_count) that has the signature of one substitution is fixed when exactly one other base makes the k-mer next
        to the solid ones solid.  Bytes that are not fixed stay as given.  min_count "auto" takes the valley of the
        spectrum at this k and these strands (256 bins) and raises ValueError when the spectrum has none.  Returns
        (reads, info): the reads as a list of bytes and a structured array of flags (CORRECT_SHORT / CLEAN / FIXED /
        WEAK), fixes, weak_before, weak_after."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        if isinstance(min_count, str):
            if min_count != "auto":
                raise ValueError('min_count must be a number or "auto"')
            min_count = self.spectrum(k, strands=strands, bins=256).threshold()["valley"]
            if not min_count:
                raise ValueError(f"min_count=\"auto\": the {k}-mer spectrum of the collection has no valley")
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        opts = _lib.DebwtFmCorrectOpts(k=int(k), min_count=int(min_count), max_rounds=int(rounds),
                                       flags=SEARCH_BOTH_STRANDS if strands == "both" else 0)
        out = ctypes.create_string_buffer(max(len(buf), 1))
        info = np.zeros(max(npat, 1), dtype=_CORRECT_DTYPE)
        self._chk(self._L.debwt_fm_correct(self._h, buf, _p64(offs), npat, ctypes.byref(opts), out,
                                           info.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmCorrectInfo))))
        raw = out.raw
        return [raw[int(offs[i]):int(offs[i + 1])] for i in range(npat)], info[:npat]

    def correct_stats(self):
        """What the last correct call did (debwt_fm_correct_stats_get): the counters of kmer_stats over all its kernels,
        rounds, reads that got a fix and ms per round, trials, fixes and reads per flag."""
        st = _lib.DebwtFmCorrectStats()
        self._chk(self._L.debwt_fm_correct_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def string_graph(self, min_overlap=20, reduce=True):
        """The string graph of the indexed records (debwt_fm_string_graph): per record kept, duplicate (an earlier record
        is equal) or contained (a substring of a longer record); among the kept records the longest suffix-prefix overlap
        of at least min_overlap per ordered pair, strand 0; with reduce the transitive edges are dropped.  An index
        without a text restores it first.  Returns a GraphResult."""
        return GraphResult(self, *self._graph_call(self._L.debwt_fm_string_graph, self.nrec, min_overlap, reduce))

    def _graph_call(self, fn, nn, min_overlap, reduce):
        """(state, offsets, edges, reduced) of a string-graph call over nn nodes"""
        flags = 0 if reduce else GRAPH_ALL_EDGES
        state = np.zeros(max(nn, 1), dtype=np.uint8)
        offs = np.zeros(nn + 1, dtype=np.uint64)
        cap = 4 * nn + 16                                     # first estimate; grown to the exact count on DEBWT_ERANGE
        while True:
            edges = np.zeros(cap, dtype=_EDGE_DTYPE)
            rc = fn(self._h, int(min_overlap), flags, state.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _p64(offs),
                    edges.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmEdge)), cap)
            if rc == -5 and int(offs[nn]) > cap:
                cap = int(offs[nn])
                continue
            self._chk(rc)
            break
        return state[:nn], offs, edges[:int(offs[nn])].copy(), bool(reduce)

    def graph_stats(self):
        """What the last string_graph() or edges_reduce() did (debwt_fm_graph_stats_get): records per state, hits walked,
        edges, reducible edges, witness lists searched, launches, scratch and edge bytes, ms per phase and wall."""
        st = _lib.DebwtFmGraphStats()
        self._chk(self._L.debwt_fm_graph_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def string_graph_both(self, min_overlap=20, reduce=True):
        """The string graph over both strands (debwt_fm_string_graph_both): the graph string_graph() gives on the doubled
        collection (S_0, rc S_0, S_1, ...), from this index alone.  Node 2r + o is read r as it is (o = 0) or
        reverse-complemented (o = 1).  Returns a BiGraphResult."""
        return BiGraphResult(self, *self._graph_call(self._L.debwt_fm_string_graph_both, 2 * self.nrec, min_overlap, reduce))

    def clean_stats(self):
        """What the last graph_clean() on this index did (debwt_fm_clean_stats_get): nodes, edges, rounds, tips clipped and
        their nodes, branches popped and their nodes, nodes visited by the walks, launches, ms of the kernels and wall."""
        st = _lib.DebwtFmCleanStats()
        self._chk(self._L.debwt_fm_clean_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def graph_both_stats(self):
        """What the last string_graph_both() did (debwt_fm_graph_both_stats_get): the fields of graph_stats() with the
        states counted in reads, self-rc reads, tail seeds, seed rows located, tail hits verified, the edges of E per kind
        (++, +-, -+, --) and ms of the tail search and of the merge beside the other phases."""
        st = _lib.DebwtFmGraphBothStats()
        self._chk(self._L.debwt_fm_graph_both_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def attach_text(self, source=None, words=None, sep=None):
        """Give the index its text (debwt_fm_attach_text; n / 4 bytes of HBM), which extend() and map() read.  source: the
        DeBWT context the index was made from (device-to-device copy), or None with the host text words / sep as
        pack_records() and pack_fasta() return them (the path after FMIndex.open).  A text that is not the index's raises."""
        if source is not None:
            self._chk(self._L.debwt_fm_attach_text(self._h, source._h, None, None))
            return
        if words is None or sep is None:
            raise ValueError("attach_text needs a DeBWT context or the packed words and separator positions")
        words = np.ascontiguousarray(words, dtype=np.uint64)
        sep = np.ascontiguousarray(sep, dtype=np.uint64)
        if len(sep) != self.nrec or len(words) < (self.n + 63) // 32:
            raise DebwtError(-1, "the text has another number of records or fewer words than the index's n asks for")
        self._chk(self._L.debwt_fm_attach_text(self._h, None, _p64(words), _p64(sep)))

    def restore_text(self):
        """Rebuild the 2-bit text from the index alone and attach it (debwt_fm_restore_text): attach_text() without a
        source, for an index opened from its files.  Returns at once when a text is attached; raises DEBWT_EINVAL, with no
        text attached, when the samples are not those of the rows."""
        self._chk(self._L.debwt_fm_restore_text(self._h))

    def text(self):
        """The attached text on the host (debwt_fm_text_fetch): (words, sep) as pack_records() returns them, ((n + 63) >> 5)
        + 2 words and the nrec separator positions -- DeBWT.load_packed(words, n, sep) takes them."""
        words = np.zeros(((self.n + 63) >> 5) + 2, dtype=np.uint64)
        sep = np.zeros(self.nrec, dtype=np.uint64)
        self._chk(self._L.debwt_fm_text_fetch(self._h, _p64(words), len(words), _p64(sep)))
        return words, sep

    def extract(self, jobs):
        """Record text from the index alone (debwt_fm_extract).  jobs: (record, offset, length) or (record,) for a whole
        record; a length past the record's end is clipped.  Returns a list of bytes, upper-case ACGT."""
        jobs = [tuple(int(x) for x in j) for j in jobs]
        nj = len(jobs)
        ja = (_lib.DebwtFmExtractJob * max(nj, 1))()
        for k, j in enumerate(jobs):
            rec, off, length = j if len(j) == 3 else (j[0], 0, 2 ** 64 - 1)
            if not (0 <= rec < 2 ** 32 and 0 <= off < 2 ** 64 and 0 <= length < 2 ** 64):
                raise DebwtError(-1, "a job with a negative or oversized field")
            ja[k].record, ja[k].reserved, ja[k].offset, ja[k].length = rec, 0, off, length
        offs = np.zeros(nj + 1, dtype=np.uint64)
        rc = self._L.debwt_fm_extract(self._h, ja, nj, _p64(offs), None, 0)      # the lengths first
        if rc != -5:
            self._chk(rc)
        total = int(offs[nj])
        buf = ctypes.create_string_buffer(max(total, 1))
        if total:
            self._chk(self._L.debwt_fm_extract(self._h, ja, nj, _p64(offs), buf, total))
        raw = buf.raw
        return [raw[int(offs[k]):int(offs[k + 1])] for k in range(nj)]

    def extract_stats(self):
        """What the last extract() or restore_text() did (debwt_fm_extract_stats_get): jobs, batches, segments, bases, LF
        steps and wave steps, the anchors' bytes and the ms to build them, kernel and wall ms."""
        st = _lib.DebwtFmExtractStats()
        self._chk(self._L.debwt_fm_extract_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def extend(self, patterns, jobs, scoring=(1, 4, 6, 1), band=16, cigar=True):
        """Banded affine-gap local alignment of jobs (debwt_fm_extend).  jobs: rows of (pattern index, strand, diag, record),
        diag = text position - query position, the query being the pattern (strand 0) or its reverse complement (strand 1).
        scoring: (match, mismatch, gap open, gap extend), a gap of length L costs open + L * extend; band: half-width 0..63.
        cigar=False: scores and alignment ends only (no traceback).  Returns an ExtendResult."""
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        jobs = [tuple(int(x) for x in j) for j in jobs]
        nj = len(jobs)
        ja = (_lib.DebwtFmJob * max(nj, 1))()
        for k, (p, s, d, r) in enumerate(jobs):
            if p < 0 or s < 0 or r < 0 or r >= 2 ** 32 or s >= 2 ** 32:
                raise DebwtError(-1, "a job with a negative or oversized field")
            ja[k].pattern, ja[k].strand, ja[k].diag, ja[k].record = p, s, d, r
        sc = _lib.DebwtFmScoring(*[int(x) for x in scoring])
        out = np.zeros(max(nj, 1), dtype=_ALN_DTYPE)
        outp = out.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmAln))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if not cigar:
            self._chk(self._L.debwt_fm_extend(self._h, buf, _p64(offs), npat, ja, nj, ctypes.byref(sc), int(band), outp, None,
                                              None, 0))
            return ExtendResult(out[:nj], None, None)
        coff = np.zeros(nj + 1, dtype=np.uint64)
        cap = 4 * nj + 16
        while True:
            cg = np.zeros(cap, dtype=np.uint32)
            rc = self._L.debwt_fm_extend(self._h, buf, _p64(offs), npat, ja, nj, ctypes.byref(sc), int(band), outp, _p64(coff),
                                         cg.ctypes.data_as(u32p), cap)
            if rc == -5 and int(coff[nj]) > cap:
                cap = int(coff[nj])
                continue
            self._chk(rc)
            break
        return ExtendResult(out[:nj], coff, cg[:int(coff[nj])].copy())

    def extend_stats(self):
        """What the last extend() (or the extension stage of the last map()) did (debwt_fm_extend_stats_get)."""
        st = _lib.DebwtFmExtendStats()
        self._chk(self._L.debwt_fm_extend_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def map(self, patterns, min_len=19, band=16, max_occ=64, max_cand=8, min_score=30, scoring=(1, 4, 6, 1), strands="both"):
        """Reads to alignments (debwt_fm_map): MEM seeds of at least min_len, at most max_occ occurrences of each, clustered
        by diagonal within `band`, the max_cand heaviest clusters extended, the best score kept; mapq = 60 * (score - sub) /
        score.  A plain heuristic, not BWA-MEM's.  Needs attach_text().  Returns a MapResult."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        o = _lib.DebwtFmMapOpts()
        self._L.debwt_fm_map_defaults(ctypes.byref(o))
        o.min_len, o.band, o.max_occ, o.max_cand, o.min_score = int(min_len), int(band), int(max_occ), int(max_cand), int(min_score)
        o.flags = MAP_FORWARD if strands == "forward" else 0
        o.scoring = _lib.DebwtFmScoring(*[int(x) for x in scoring])
        hits = np.zeros(max(npat, 1), dtype=_HIT_DTYPE)
        coff = np.zeros(npat + 1, dtype=np.uint64)
        cap = 4 * npat + 16
        while True:
            cg = np.zeros(cap, dtype=np.uint32)
            rc = self._L.debwt_fm_map(self._h, buf, _p64(offs), npat, ctypes.byref(o),
                                      hits.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmHit)), _p64(coff),
                                      cg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap)
            if rc == -5 and int(coff[npat]) > cap:
                cap = int(coff[npat])
                continue
            self._chk(rc)
            break
        return MapResult(hits[:npat], coff, cg[:int(coff[npat])].copy())

    def extend_chain(self, patterns, jobs, anchors, scoring=(1, 4, 6, 1), band=16, cigar=True):
        """Banded affine-gap local alignment along chains (debwt_fm_extend_chain): as extend(), but the band of query row i
        is centred on the diagonal of the job's last anchor at or before i.  jobs: rows of (pattern index, strand, record,
        first anchor, number of anchors); anchors: rows of (qbeg, diag), qbeg strictly increasing inside a job and
        consecutive diag at most `band` apart.  A job with one anchor is an extend() job.  Returns an ExtendResult."""
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        jobs = [tuple(int(x) for x in j) for j in jobs]
        anchors = [tuple(int(x) for x in a) for a in anchors]
        nj, na = len(jobs), len(anchors)
        ja = (_lib.DebwtFmChainJob * max(nj, 1))()
        for k, (p, s, r, fa, n) in enumerate(jobs):
            if min(p, s, r, fa, n) < 0 or max(s, r, n) >= 2 ** 32:
                raise DebwtError(-1, "a job with a negative or oversized field")
            ja[k].pattern, ja[k].strand, ja[k].record, ja[k].first_anchor, ja[k].n_anchors = p, s, r, fa, n
        aa = (_lib.DebwtFmAnchor * max(na, 1))()
        for k, (q, d) in enumerate(anchors):
            if q < 0 or q >= 2 ** 32:
                raise DebwtError(-1, "an anchor with a negative or oversized qbeg")
            aa[k].qbeg, aa[k].diag = q, d
        sc = _lib.DebwtFmScoring(*[int(x) for x in scoring])
        out = np.zeros(max(nj, 1), dtype=_ALN_DTYPE)
        outp = out.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmAln))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if not cigar:
            self._chk(self._L.debwt_fm_extend_chain(self._h, buf, _p64(offs), npat, ja, nj, aa, na, ctypes.byref(sc), int(band),
                                                    outp, None, None, 0))
            return ExtendResult(out[:nj], None, None)
        coff = np.zeros(nj + 1, dtype=np.uint64)
        cap = 4 * nj + 16
        while True:
            cg = np.zeros(cap, dtype=np.uint32)
            rc = self._L.debwt_fm_extend_chain(self._h, buf, _p64(offs), npat, ja, nj, aa, na, ctypes.byref(sc), int(band), outp,
                                               _p64(coff), cg.ctypes.data_as(u32p), cap)
            if rc == -5 and int(coff[nj]) > cap:
                cap = int(coff[nj])
                continue
            self._chk(rc)
            break
        return ExtendResult(out[:nj], coff, cg[:int(coff[nj])].copy())

    def map_chained(self, patterns, min_len=19, band=16, max_occ=64, max_cand=8, min_score=30, scoring=(1, 4, 6, 1),
                    strands="both", max_gap=None):
        """Reads to alignments through chains (debwt_fm_map_chained): as map(), but the seeds of a read are chained across
        diagonals (chain_seeds with `band` and max_gap, the max_cand best chains kept) and each chain is extended with a
        band that follows it (extend_chain).  Returns a MapResult whose anchors(i) are the winning chain's (qbeg, diag)."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        co = _lib.DebwtFmChainOpts()
        self._L.debwt_fm_chain_defaults(ctypes.byref(co))
        o = co.map
        o.min_len, o.band, o.max_occ, o.max_cand, o.min_score = int(min_len), int(band), int(max_occ), int(max_cand), int(min_score)
        o.flags = MAP_FORWARD if strands == "forward" else 0
        o.scoring = _lib.DebwtFmScoring(*[int(x) for x in scoring])
        if max_gap is not None:
            co.max_gap = int(max_gap)
        hits = np.zeros(max(npat, 1), dtype=_HIT_DTYPE)
        coff = np.zeros(npat + 1, dtype=np.uint64)
        aoff = np.zeros(npat + 1, dtype=np.uint64)
        cap, acap = 4 * npat + 16, 4 * npat + 16
        while True:
            cg = np.zeros(cap, dtype=np.uint32)
            an = np.zeros(acap, dtype=_ANCHOR_DTYPE)
            rc = self._L.debwt_fm_map_chained(self._h, buf, _p64(offs), npat, ctypes.byref(co),
                                              hits.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmHit)), _p64(coff),
                                              cg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap, _p64(aoff),
                                              an.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmAnchor)), acap)
            if rc == -5 and (int(coff[npat]) > cap or int(aoff[npat]) > acap):
                cap, acap = max(cap, int(coff[npat])), max(acap, int(aoff[npat]))
                continue
            self._chk(rc)
            break
        return MapResult(hits[:npat], coff, cg[:int(coff[npat])].copy(), aoff, an[:int(aoff[npat])].copy())

    def align_window(self, patterns, jobs, scoring=(1, 4, 6, 1), cigar=True):
        """Affine-gap local alignment of jobs against text windows, without a band (debwt_fm_align_window).  jobs: rows of
        (pattern index, strand, record, wbeg, wend); the query -- the pattern (strand 0) or its reverse complement (strand
        1), at most 4096 bases -- is aligned against the global text positions [wbeg, wend) (at most 16384) clipped to the
        record.  Everything else is as extend() has it.  Returns an ExtendResult."""
        buf, offs = _patterns(patterns)
        npat = len(offs) - 1
        jobs = [tuple(int(x) for x in j) for j in jobs]
        nj = len(jobs)
        ja = (_lib.DebwtFmWindowJob * max(nj, 1))()
        for k, (p, s, r, b, e) in enumerate(jobs):
            if min(p, s, r, b, e) < 0 or max(s, r) >= 2 ** 32 or max(p, b, e) >= 2 ** 64:
                raise DebwtError(-1, "a job with a negative or oversized field")
            ja[k].pattern, ja[k].strand, ja[k].record, ja[k].wbeg, ja[k].wend = p, s, r, b, e
        sc = _lib.DebwtFmScoring(*[int(x) for x in scoring])
        out = np.zeros(max(nj, 1), dtype=_ALN_DTYPE)
        outp = out.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmAln))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if not cigar:
            self._chk(self._L.debwt_fm_align_window(self._h, buf, _p64(offs), npat, ja, nj, ctypes.byref(sc), outp, None,
                                                    None, 0))
            return ExtendResult(out[:nj], None, None)
        coff = np.zeros(nj + 1, dtype=np.uint64)
        cap = 4 * nj + 16
        while True:
            cg = np.zeros(cap, dtype=np.uint32)
            rc = self._L.debwt_fm_align_window(self._h, buf, _p64(offs), npat, ja, nj, ctypes.byref(sc), outp, _p64(coff),
                                               cg.ctypes.data_as(u32p), cap)
            if rc == -5 and int(coff[nj]) > cap:
                cap = int(coff[nj])
                continue
            self._chk(rc)
            break
        return ExtendResult(out[:nj], coff, cg[:int(coff[nj])].copy())

    def map_pairs(self, reads1, reads2, insert=None, max_rescue=4, unpaired_penalty=17, min_len=19, band=16, max_occ=64,
                  max_cand=8, min_score=30, scoring=(1, 4, 6, 1), strands="both"):
        """Paired-end reads to alignments (debwt_fm_map_pairs): the candidates of map() for every read, insert-size bounds
        (insert=(lo, hi), or None to estimate them from the pairs that map uniquely), the rescue of a mate in the window its
        partner's candidates leave it (align_window; max_rescue=0: none), and the choice of the pair.  reads1[p] and
        reads2[p] are the mates of pair p.  Returns a MapResult over the 2 * npairs reads in the order mate 1, mate 2 of
        pair 0, mate 1 of pair 1, ... (flags also MAP_PROPER, MAP_RESCUED); its .pairs holds tlen, pair_score and pair_sub
        of every pair.  strands: pairs are mapped on both strands; "forward" is passed on and refused by the library."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        r1 = [reads1] if isinstance(reads1, (str, bytes, bytearray)) else list(reads1)
        r2 = [reads2] if isinstance(reads2, (str, bytes, bytearray)) else list(reads2)
        if len(r1) != len(r2):
            raise ValueError("reads1 and reads2 must have the same number of reads")
        buf, offs = _patterns([r for pr in zip(r1, r2) for r in pr])
        npairs, npat = len(r1), 2 * len(r1)
        po = _lib.DebwtFmPairOpts()
        self._L.debwt_fm_pair_defaults(ctypes.byref(po))
        o = po.map
        o.min_len, o.band, o.max_occ, o.max_cand, o.min_score = int(min_len), int(band), int(max_occ), int(max_cand), int(min_score)
        o.flags = MAP_FORWARD if strands == "forward" else 0
        o.scoring = _lib.DebwtFmScoring(*[int(x) for x in scoring])
        if insert is not None:
            po.ins_lo, po.ins_hi = int(insert[0]), int(insert[1])
        po.max_rescue, po.unpaired_penalty = int(max_rescue), int(unpaired_penalty)
        hits = np.zeros(max(npat, 1), dtype=_HIT_DTYPE)
        info = np.zeros(max(npairs, 1), dtype=_PAIR_DTYPE)
        coff = np.zeros(npat + 1, dtype=np.uint64)
        cap = 4 * npat + 16
        while True:
            cg = np.zeros(cap, dtype=np.uint32)
            rc = self._L.debwt_fm_map_pairs(self._h, buf, _p64(offs), npairs, ctypes.byref(po),
                                            hits.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmHit)),
                                            info.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmPairInfo)), _p64(coff),
                                            cg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap)
            if rc == -5 and int(coff[npat]) > cap:
                cap = int(coff[npat])
                continue
            self._chk(rc)
            break
        res = MapResult(hits[:npat], coff, cg[:int(coff[npat])].copy())
        res.pairs = info[:npairs]
        return res

    def pair_stats(self):
        """Counts, the insert bounds used and the stage times of the last map_pairs() (debwt_fm_pair_stats_get)."""
        st = _lib.DebwtFmPairStats()
        self._chk(self._L.debwt_fm_pair_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def map_stats(self):
        """Stage times and counts of the last map() or map_chained() (debwt_fm_map_stats_get)."""
        st = _lib.DebwtFmMapStats()
        self._chk(self._L.debwt_fm_map_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def pileup(self, patterns, alns, window=None, add=False):
        """Pile alignments up into per-position counts (debwt_fm_pileup, definition 7 of debwt_hip.h).  alns: (rows, offsets,
        cigars) -- rows of (pattern, tbeg, qbeg, strand) or an array of _PILE_ALN_DTYPE, and the BAM-coded CIGARs as
        extend() and map() return them; MapResult.pileup and ExtendResult.pileup build it.  window: (wbeg, wend) global
        text positions, None for the whole text.  add=True adds to the resident table of the same window instead of
        clearing it, so reads can arrive in batches.  The table stays on the device; returns a PileupResult."""
        buf, offs = _patterns(patterns)
        rows, coff, cg = _pile_alns(alns)
        wbeg, wend = (0, self.n) if window is None else (int(window[0]), int(window[1]))
        if wbeg < 0 or wend < 0:
            raise DebwtError(-1, "a negative window bound")
        self._chk(self._L.debwt_fm_pileup(self._h, buf, _p64(offs), len(offs) - 1,
                                          rows.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmPileAln)), len(coff) - 1, _p64(coff),
                                          cg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), wbeg, wend,
                                          PILE_ADD if add else 0))
        return PileupResult(self, buf, offs, (rows[:len(coff) - 1], coff, cg), (wbeg, wend))

    def pile_fetch(self):
        """The resident table (debwt_fm_pile_fetch): ((wbeg, wend), counts) with counts W x 8 uint32 -- A, C, G, T,
        deletions, insertions anchored here, other characters, unused."""
        win = np.zeros(2, dtype=np.uint64)
        rc = self._L.debwt_fm_pile_fetch(self._h, _p64(win), None, 0)
        if rc != -5:
            self._chk(rc)
        W = int(win[1] - win[0])
        counts = np.zeros((W, 8), dtype=np.uint32)
        self._chk(self._L.debwt_fm_pile_fetch(self._h, _p64(win), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), W))
        return (int(win[0]), int(win[1])), counts

    def pile_release(self):
        """Free the resident table (debwt_fm_pile_release)."""
        self._chk(self._L.debwt_fm_pile_release(self._h))

    def pile_call(self, min_depth=4, min_permille=600):
        """Definition 8 on the resident table (debwt_fm_pile_call): (calls, ref, variants).  min_depth and min_permille are
        knobs, not measurements."""
        win = np.zeros(2, dtype=np.uint64)
        rc = self._L.debwt_fm_pile_fetch(self._h, _p64(win), None, 0)
        if rc != -5:
            self._chk(rc)
        W = int(win[1] - win[0])
        o = _lib.DebwtFmPileOpts(int(min_depth), int(min_permille))
        calls, ref = np.zeros(W, dtype=np.uint8), np.zeros(W, dtype=np.uint8)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        nv = ctypes.c_uint64(0)
        var = np.zeros(1, dtype=_VARIANT_DTYPE)
        rc = self._L.debwt_fm_pile_call(self._h, ctypes.byref(o), calls.ctypes.data_as(u8p), ref.ctypes.data_as(u8p),
                                        var.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmVariant)), 0, ctypes.byref(nv))
        if rc == -5 and nv.value:
            var = np.zeros(nv.value, dtype=_VARIANT_DTYPE)
            rc = self._L.debwt_fm_pile_call(self._h, ctypes.byref(o), calls.ctypes.data_as(u8p), ref.ctypes.data_as(u8p),
                                            var.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmVariant)), len(var), ctypes.byref(nv))
        self._chk(rc)
        return calls, ref, var[:nv.value]

    def pile_insertions(self, patterns, alns, positions):
        """The I ops of the alignments anchored at one of `positions` (ascending), as an array of (t, aln, qpos, len)
        ordered by (t, aln, qpos) (debwt_fm_pile_insertions)."""
        _, offs = _patterns(patterns)
        rows, coff, cg = _pile_alns(alns)
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        ne = ctypes.c_uint64(0)
        ev = np.zeros(1, dtype=_INS_EVENT_DTYPE)
        args = (self._h, len(offs) - 1, _p64(offs), rows.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmPileAln)), len(coff) - 1,
                _p64(coff), cg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _p64(pos) if len(pos) else None, len(pos))
        rc = self._L.debwt_fm_pile_insertions(*args, ev.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmInsEvent)), 0, ctypes.byref(ne))
        if rc == -5 and ne.value:
            ev = np.zeros(ne.value, dtype=_INS_EVENT_DTYPE)
            rc = self._L.debwt_fm_pile_insertions(*args, ev.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmInsEvent)), len(ev),
                                                  ctypes.byref(ne))
        self._chk(rc)
        return ev[:ne.value]

    def pile_stats(self):
        """What the last pileup() and the last call on its table did (debwt_fm_pile_stats_get)."""
        st = _lib.DebwtFmPileStats()
        self._chk(self._L.debwt_fm_pile_stats_get(self._h, ctypes.byref(st)))
        return st.as_dict()

    def locate_hits(self, result, max_per_pattern=None):
        """Text positions of a SearchResult's hits (debwt_fm_locate on its ranges): per pattern a tuple of uint64
        positions, uint8 strands and uint8 mismatches, ascending by (position, strand).  max_per_pattern caps the rows
        taken per pattern, in hit order (strand, mismatches, row)."""
        r = result.ranges
        cnt = (r[:, 1] - r[:, 0]).astype(np.uint64) if len(r) else np.zeros(0, dtype=np.uint64)
        npat = len(result.offsets) - 1
        if max_per_pattern is not None and len(r):
            pat = np.repeat(np.arange(npat), np.diff(result.offsets).astype(np.int64))
            excl = np.zeros(len(cnt) + 1, dtype=np.int64)
            np.cumsum(cnt.astype(np.int64), out=excl[1:])
            before = excl[:-1] - excl[result.offsets[:-1].astype(np.int64)[pat]]    # rows of the pattern's earlier hits
            cnt = np.minimum(cnt.astype(np.int64), np.maximum(int(max_per_pattern) - before, 0)).astype(np.uint64)
        rr = np.ascontiguousarray(np.stack([r[:, 0], r[:, 0] + cnt], axis=1) if len(r) else np.zeros((0, 2), np.uint64),
                                  dtype=np.uint64)
        total = int(cnt.sum())
        offs = np.zeros(len(rr) + 1, dtype=np.uint64)
        pos = np.empty(max(total, 1), dtype=np.uint64)
        if len(rr):
            self._chk(self._L.debwt_fm_locate(self._h, _p64(rr), len(rr), 0, _p64(offs), _p64(pos), len(pos)))
        pos = pos[:total]
        per_hit = cnt.astype(np.int64)
        strand = np.repeat(result.strands, per_hit)
        mism = np.repeat(result.mismatches, per_hit)
        out = []
        for i in range(npat):
            a, b = int(offs[int(result.offsets[i])]), int(offs[int(result.offsets[i + 1])])
            p, s, m = pos[a:b], strand[a:b], mism[a:b]
            o = np.lexsort((s, p))
            out.append((p[o], s[o], m[o]))
        return out


SEARCH_BOTH_STRANDS, SEARCH_BEST_ONLY = 1, 2
MAP_REVERSE, MAP_UNMAPPED, MAP_TOO_LONG = 1, 2, 4      # MapResult.flags
MAP_PROPER, MAP_RESCUED = 8, 16                        # MapResult.flags of FMIndex.map_pairs
MAP_FORWARD = 1                                        # option flag of debwt_fm_map
OVERLAP_LONGEST = 2                                    # option flag of debwt_fm_overlaps
OVERLAP_CONTAINS, OVERLAP_WHOLE = 1, 2                 # OverlapResult hit flags
ESA_SA, ESA_DA = 1, 2                                  # flags of debwt_fm_esa_build
REPEAT_KINDS = {"maximal": 0, "supermaximal": 1, "intervals": 2}                 # kind of debwt_fm_repeats
RECORDS_UNIQUE = 1                                                                # flags of debwt_fm_record_filter
REPEAT_IS_MAXIMAL, REPEAT_IS_SUPERMAXIMAL = 1, 2       # flags of a repeat
REPEAT_DTYPE = np.dtype([("row_lo", "<u8"), ("count", "<u8"), ("left", "<u8", (5,)), ("len", "<u4"), ("flags", "<u4")])
CDBG_CIRCULAR = 1                                      # flags of a unitig of debwt_fm_cdbg
UNITIG_DTYPE = np.dtype([("row_lo", "<u8"), ("seq_offset", "<u8"), ("kmer_count", "<u8"), ("nodes", "<u4"), ("flags", "<u4")])
CDBG_EDGE_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4")])
CORRECT_SHORT, CORRECT_CLEAN, CORRECT_FIXED, CORRECT_WEAK = 1, 2, 4, 8   # flags of FMIndex.correct's info
_CORRECT_DTYPE = np.dtype([("flags", np.uint32), ("fixes", np.uint32), ("weak_before", np.uint32), ("weak_after", np.uint32)])
_TRIAL_DTYPE = np.dtype([("run_a", np.uint32), ("run_b", np.uint32), ("pos", np.uint32), ("window", np.uint32),
                         ("kind", np.uint32)])
_OVERLAP_DTYPE = np.dtype([("record", np.uint32), ("length", np.uint32), ("strand", np.uint32), ("flags", np.uint32)])
GRAPH_ALL_EDGES = 1                                    # option flag of debwt_fm_string_graph
NODE_KEPT, NODE_DUPLICATE, NODE_CONTAINED = 0, 1, 2    # GraphResult.state
NODE_CLIPPED, NODE_POPPED = 3, 4                       # states that graph_clean() writes: in a tip, in a popped branch
CLEAN_MIRRORED = 1                                     # option flag of debwt_fm_graph_clean
_EDGE_DTYPE = np.dtype([("record", np.uint32), ("length", np.uint32)])
_ALN_DTYPE = np.dtype([("score", np.int32), ("qbeg", np.uint32), ("qend", np.uint32), ("edits", np.uint32),
                       ("tbeg", np.uint64), ("tend", np.uint64)])
_HIT_DTYPE = np.dtype([("pattern", np.uint64), ("flags", np.uint32), ("record", np.uint32), ("offset", np.uint64),
                       ("qbeg", np.uint32), ("qend", np.uint32), ("tbeg", np.uint64), ("tend", np.uint64),
                       ("score", np.int32), ("sub", np.int32), ("mapq", np.uint32), ("edits", np.uint32),
                       ("diag", np.int64)])
PILE_ADD = 1                                           # option flag of debwt_fm_pileup
PILE_NO_CALL, PILE_DELETION, PILE_INS_BIT = 5, 4, 0x10   # call bytes of debwt_fm_pile_call
_PILE_ALN_DTYPE = np.dtype([("pattern", np.uint64), ("tbeg", np.uint64), ("qbeg", np.uint32), ("strand", np.uint32)])
_VARIANT_DTYPE = np.dtype([("t", np.uint64), ("depth", np.uint32), ("count", np.uint32), ("ins", np.uint32),
                           ("ref", np.uint8), ("call", np.uint8)], align=True)
_INS_EVENT_DTYPE = np.dtype([("t", np.uint64), ("aln", np.uint64), ("qpos", np.uint32), ("len", np.uint32)])
_ANCHOR_DTYPE = np.dtype([("qbeg", np.uint32), ("reserved", np.uint32), ("diag", np.int64)])
_PAIR_DTYPE = np.dtype([("tlen", np.int64), ("pair_score", np.int32), ("pair_sub", np.int32), ("reserved", np.uint32)],
                       align=True)


def cigar_string(ops):
    """BAM-coded ops (len << 4 | op, M 0, I 1, D 2) as text"""
    return "".join(f"{int(x) >> 4}{'MID'[int(x) & 15]}" for x in ops)


def cluster_seeds(seeds, band=16, max_cand=8):
    """Seeds of one read to extension candidates on the host (debwt_fm_cluster_seeds, no GPU).  seeds: rows of (strand,
    record, diag, qbeg, qend).  Returns dicts (strand, record, diag, first_diag, weight, seeds), heaviest first."""
    L = _lib.lib()
    seeds = list(seeds)
    sa = (_lib.DebwtFmSeed * max(len(seeds), 1))()
    for k, (st, rec, dg, qb, qe) in enumerate(seeds):
        sa[k].strand, sa[k].record, sa[k].diag, sa[k].qbeg, sa[k].qend = int(st), int(rec), int(dg), int(qb), int(qe)
    out = (_lib.DebwtFmCand * max(int(max_cand), 1))()
    rc = L.debwt_fm_cluster_seeds(sa, len(seeds), int(band), int(max_cand), out)
    if rc < 0:
        raise DebwtError(rc)
    return [{n: int(getattr(out[k], n)) for n, _ in _lib.DebwtFmCand._fields_} for k in range(rc)]


def weak_trials(counts, k, min_count):
    """Weak runs and trials of one read's k-mer counts on the host (debwt_fm_weak_trials, no GPU): a structured array of
    (run_a, run_b, pos, window, kind) with kind 0 = left, 1 = right, runs ascending, left first."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    L = _lib.lib()
    p = c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if len(c) else None
    n = L.debwt_fm_weak_trials(p, len(c), int(k), int(min_count), None, 0)
    if n < 0:
        raise DebwtError(n)
    out = np.zeros(n, dtype=_TRIAL_DTYPE)
    if n:
        rc = L.debwt_fm_weak_trials(p, len(c), int(k), int(min_count), out.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmTrial)), n)
        if rc != n:
            raise DebwtError(rc if rc < 0 else -6)
    return out


def spectrum_threshold(hist, total):
    """Valley, peak and size estimate of a k-mer spectrum on the host (debwt_fm_spectrum_threshold, no GPU): valley = the
    smallest c in 1..bins-3 with hist[c + 1] > hist[c], peak = the fullest bin in valley+1..bins-2 (the smallest on ties),
    est_size = (total - the k-mers below the valley) // peak; all 0 when the histogram has no valley."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    out = _lib.DebwtFmSpectrumSummary()
    rc = _lib.lib().debwt_fm_spectrum_threshold(_p64(h) if len(h) else None, len(h), int(total), ctypes.byref(out))
    if rc:
        raise DebwtError(rc)
    return {"valley": int(out.valley), "peak": int(out.peak), "est_size": int(out.est_size)}


def kmer_string(code, k):
    """The letters of a k-mer code (A, C, G, T = 0..3, the first character in the most significant digit)."""
    code, k = int(code), int(k)
    if not 1 <= k <= 32 or not 0 <= code < 4 ** k:
        raise ValueError("k must be 1..32 and the code below 4^k")
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def overlap_longest(hits, offsets):
    """The reduction of overlaps(longest=True) on the host (debwt_fm_overlap_longest, no GPU): hits (structured array of
    record, length, strand, flags) in the order of OverlapResult, pattern i's in offsets[i] .. offsets[i + 1]; per
    (pattern, strand, record) the longest stays.  Returns (hits, offsets) of the reduced list; input that is not in that
    order raises DebwtError (DEBWT_EINVAL)."""
    h = np.array(hits, dtype=_OVERLAP_DTYPE, copy=True)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offs) < 1 or int(offs[-1]) > len(h):
        raise ValueError("offsets do not fit the hits")
    out = np.zeros(len(offs), dtype=np.uint64)
    rc = _lib.lib().debwt_fm_overlap_longest(h.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmOverlap)), _p64(offs), len(offs) - 1,
                                             _p64(out))
    if rc:
        raise DebwtError(rc)
    return h[int(out[0]):int(out[-1])].copy(), out - out[0]


def chain_seeds(seeds, band=16, max_gap=5000, max_chains=8):
    """Seeds of one read to colinear chains on the host (debwt_fm_chain_seeds, no GPU).  seeds: rows of (strand, record,
    diag, qbeg, qend).  Returns dicts (score, strand, record, anchors: the chain's (qbeg, diag) in ascending qbeg), the
    best score first."""
    L = _lib.lib()
    seeds = list(seeds)
    sa = (_lib.DebwtFmSeed * max(len(seeds), 1))()
    for k, (st, rec, dg, qb, qe) in enumerate(seeds):
        sa[k].strand, sa[k].record, sa[k].diag, sa[k].qbeg, sa[k].qend = int(st), int(rec), int(dg), int(qb), int(qe)
    ch = (_lib.DebwtFmChain * max(int(max_chains), 1))()
    an = (_lib.DebwtFmAnchor * max(len(seeds), 1))()                       # chains share no seed
    need = ctypes.c_uint64(0)
    rc = L.debwt_fm_chain_seeds(sa, len(seeds), int(band), int(max_gap), int(max_chains), ch, an, len(seeds), ctypes.byref(need))
    if rc < 0:
        raise DebwtError(rc)
    return [{"score": int(ch[k].score), "strand": int(ch[k].strand), "record": int(ch[k].record),
             "anchors": [(int(an[x].qbeg), int(an[x].diag))
                         for x in range(int(ch[k].first_anchor), int(ch[k].first_anchor) + int(ch[k].n_anchors))]}
            for k in range(rc)]


def insert_bounds(tlens):
    """(lo, hi) insert-size bounds from observed template lengths on the host (debwt_fm_insert_bounds, no GPU): with
    the quartiles q1, q3 of the sorted values and d = q3 - q1, lo = max(1, q1 - 3 d) and hi = min(16384, q3 + 3 d).
    Fewer than 32 values raise."""
    L = _lib.lib()
    t = np.ascontiguousarray(tlens, dtype=np.uint64)
    lo, hi = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = L.debwt_fm_insert_bounds(_p64(t) if len(t) else None, len(t), ctypes.byref(lo), ctypes.byref(hi))
    if rc < 0:
        raise DebwtError(rc)
    return int(lo.value), int(hi.value)


def pair_select(c1, c2, ins_lo, ins_hi, unpaired_penalty=17, min_score=30):
    """The choice of one pair from the candidates of its mates on the host (debwt_fm_pair_select, no GPU).  c1, c2: rows
    of (score, record, strand, tbeg, tend).  Returns a dict (i1, i2, proper, mapq1, mapq2, sub1, sub2, pair_score,
    pair_sub, tlen); i1 / i2 = -1: the mate has no eligible candidate."""
    L = _lib.lib()

    def arr(c):
        c = list(c)
        a = (_lib.DebwtFmPcand * max(len(c), 1))()
        for k, (sc, rec, st, tb, te) in enumerate(c):
            a[k].score, a[k].record, a[k].strand, a[k].tbeg, a[k].tend = int(sc), int(rec), int(st), int(tb), int(te)
        return a, len(c)

    (a1, n1), (a2, n2) = arr(c1), arr(c2)
    if min(int(ins_lo), int(ins_hi)) < 0:
        raise DebwtError(-1, "negative insert bounds")
    ch = _lib.DebwtFmPairChoice()
    rc = L.debwt_fm_pair_select(a1, n1, a2, n2, int(ins_lo), int(ins_hi), int(unpaired_penalty), int(min_score), ctypes.byref(ch))
    if rc < 0:
        raise DebwtError(rc)
    return {n: int(getattr(ch, n)) for n, _ in _lib.DebwtFmPairChoice._fields_}


def _pile_alns(alns):
    """(rows of _PILE_ALN_DTYPE with at least one element, cigar offsets, cigars with at least one element)"""
    rows, coff, cg = alns
    if not (isinstance(rows, np.ndarray) and rows.dtype == _PILE_ALN_DTYPE):
        lst = [tuple(int(x) for x in r) for r in rows]
        for r in lst:
            if len(r) != 4 or min(r) < 0 or r[0] >= 2 ** 64 or r[1] >= 2 ** 64 or r[2] >= 2 ** 32 or r[3] >= 2 ** 32:
                raise DebwtError(-1, "an alignment with a negative or oversized field")
        rows = np.array(lst, dtype=_PILE_ALN_DTYPE) if lst else np.zeros(0, dtype=_PILE_ALN_DTYPE)
    coff = np.ascontiguousarray(coff, dtype=np.uint64)
    if len(coff) != len(rows) + 1:
        raise ValueError("cigar offsets: one more than alignments expected")
    cg = np.ascontiguousarray(cg, dtype=np.uint32)
    if len(rows) == 0:
        rows = np.zeros(1, dtype=_PILE_ALN_DTYPE)
    if len(cg) == 0:
        cg = np.zeros(1, dtype=np.uint32)
    return np.ascontiguousarray(rows), coff, cg


def ins_vote(patterns, alns, events):
    """The vote over the insertion events of one position (debwt_fm_ins_vote, host only): (string, support).  alns: the
    alignment rows the events name; the most frequent inserted string wins, ties go to the shorter, then the smaller."""
    L = _lib.lib()
    buf, offs = _patterns(patterns)
    rows, _, _ = _pile_alns((alns, np.zeros(len(alns) + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)))
    ev = np.ascontiguousarray(events, dtype=_INS_EVENT_DTYPE)
    evp = ev.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmInsEvent)) if len(ev) else None
    n, sup = ctypes.c_uint64(0), ctypes.c_uint32(0)
    args = (buf, _p64(offs), len(offs) - 1, rows.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmPileAln)), len(alns), evp, len(ev))
    rc = L.debwt_fm_ins_vote(*args, None, 0, ctypes.byref(n), ctypes.byref(sup))
    if rc not in (0, -5):
        raise DebwtError(rc)
    out = ctypes.create_string_buffer(max(n.value, 1))
    rc = L.debwt_fm_ins_vote(*args, out, n.value, ctypes.byref(n), ctypes.byref(sup))
    if rc:
        raise DebwtError(rc)
    return out.raw[:n.value].decode(), sup.value


def consensus(ref, calls, window, insertions, rec_starts, n, min_permille=600):
    """The consensus of every record inside a window (debwt_fm_consensus, host only): a list of nrec strings.  ref, calls:
    as FMIndex.pile_call returns them; insertions: (t, string, support, depth) ascending by t."""
    L = _lib.lib()
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    calls = np.ascontiguousarray(calls, dtype=np.uint8)
    ins = sorted((int(t), s.encode() if isinstance(s, str) else bytes(s), int(sup), int(d)) for t, s, sup, d in insertions)
    it = np.array([i[0] for i in ins], dtype=np.uint64)
    ioff = np.zeros(len(ins) + 1, dtype=np.uint64)
    if ins:
        np.cumsum([len(i[1]) for i in ins], out=ioff[1:])
    isup = np.array([i[2] for i in ins], dtype=np.uint32)
    idep = np.array([i[3] for i in ins], dtype=np.uint32)
    starts = np.ascontiguousarray(rec_starts, dtype=np.uint64)
    nrec = len(starts)
    ooff = np.zeros(nrec + 1, dtype=np.uint64)
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    args = (ref.ctypes.data_as(u8p), calls.ctypes.data_as(u8p), int(window[0]), int(window[1]),
            _p64(it) if ins else None, _p64(ioff), b"".join(i[1] for i in ins), isup.ctypes.data_as(u32p) if ins else None,
            idep.ctypes.data_as(u32p) if ins else None, len(ins), int(min_permille), _p64(starts), nrec, int(n), _p64(ooff))
    rc = L.debwt_fm_consensus(*args, None, 0)
    if rc not in (0, -5):
        raise DebwtError(rc)
    total = int(ooff[nrec])
    out = ctypes.create_string_buffer(max(total, 1))
    rc = L.debwt_fm_consensus(*args, out, total)
    if rc:
        raise DebwtError(rc)
    raw = out.raw
    return [raw[int(ooff[r]):int(ooff[r + 1])].decode() for r in range(nrec)]


class PileupResult:
    """The table FMIndex.pileup left on the device: window (wbeg, wend); counts (W x 8 uint32: A, C, G, T, deletions,
    insertions anchored here, other characters, unused) and depth (the sum of the first five) are fetched on first use.
    The table belongs to the index: the next pileup() without add=True replaces it, so fetch or call before that.
    call() and consensus() see the insertions of this call's alignments only."""

    def __init__(self, index, buf, offs, alns, window):
        self.index, self.window, self.alns = index, window, alns
        self._buf, self._offs, self._counts = buf, offs, None

    @property
    def counts(self):
        if self._counts is None:
            win, self._counts = self.index.pile_fetch()
            if win != self.window:
                raise DebwtError(-4, "the resident table is no longer this result's")
        return self._counts

    @property
    def depth(self):
        return self.counts[:, :5].sum(axis=1, dtype=np.uint64)

    def call(self, min_depth=4, min_permille=600):
        calls, ref, var = self.index.pile_call(min_depth, min_permille)
        return CallResult(self, calls, ref, var, int(min_permille))

    def consensus(self, min_depth=4, min_permille=600):
        """(record, consensus string) of every record that has a base inside the window."""
        return self.call(min_depth, min_permille).consensus()


class CallResult:
    """Calls of PileupResult.call: calls and ref (uint8 per position of the window), variants (structured: t, depth, count,
    ins, ref, call), insertions() and consensus()."""

    def __init__(self, pile, calls, ref, variants, min_permille):
        self.pile, self.calls, self.ref, self.variants, self.min_permille = pile, calls, ref, variants, min_permille
        self._ins = None

    def insertions(self):
        """[(t, voted string, support, depth)] for every variant with the insertion bit, ascending by t."""
        if self._ins is None:
            p = self.pile
            flagged = self.variants[(self.variants["call"] & PILE_INS_BIT) != 0]
            ev = p.index.pile_insertions((p._buf, p._offs), p.alns, flagged["t"])
            out = []
            for v in flagged:
                s, sup = ins_vote((p._buf, p._offs), p.alns[0], ev[ev["t"] == v["t"]])
                out.append((int(v["t"]), s, sup, int(v["depth"])))
            self._ins = out
        return self._ins

    def consensus(self):
        p = self.pile
        starts = p.index.record_starts()
        seqs = consensus(self.ref, self.calls, p.window, self.insertions(), starts, p.index.n, self.min_permille)
        ends = np.append(starts[1:], np.uint64(p.index.n)) - np.uint64(1)
        return [(r, seqs[r]) for r in range(len(starts)) if max(int(starts[r]), p.window[0]) < min(int(ends[r]), p.window[1])]


def _hits_alns(res, keep):
    idx = np.flatnonzero(keep)
    rows = np.zeros(len(idx), dtype=_PILE_ALN_DTYPE)
    coff = np.zeros(len(idx) + 1, dtype=np.uint64)
    lens = (res.offsets[idx + 1] - res.offsets[idx]).astype(np.int64)
    if len(idx):
        np.cumsum(lens, out=coff[1:])
    # op k of the kept hits is op (first op of its hit) + (k - first kept op of its hit) of the result
    src = np.repeat(res.offsets[idx].astype(np.int64) - coff[:-1].astype(np.int64), lens) + np.arange(int(lens.sum()))
    cg = np.asarray(res.cigars)[src]
    return idx, rows, coff, cg.astype(np.uint32)


class ExtendResult:
    """Alignments of FMIndex.extend, one per job: numpy arrays score, qbeg, qend, tbeg, tend, edits ([qbeg, qend) in the
    query string, i.e. in the reverse complement for strand 1; [tbeg, tend) global text positions); cigar(i) as text and
    ops(i) as BAM-coded uint32 (None without a traceback).  score 0: no alignment, everything 0."""

    def __init__(self, aln, offsets, cigars):
        self.aln, self.offsets, self.cigars = aln, offsets, cigars
        for name in _ALN_DTYPE.names:
            setattr(self, name, aln[name].copy())

    def __len__(self):
        return len(self.aln)

    def ops(self, i):
        if self.offsets is None:
            return None
        return self.cigars[int(self.offsets[i]):int(self.offsets[i + 1])]

    def cigar(self, i):
        return None if self.offsets is None else cigar_string(self.ops(i))

    def alignments(self, jobs):
        """The alignments with a positive score as FMIndex.pileup takes them; jobs: the rows given to extend()."""
        if self.offsets is None:
            raise ValueError("alignments without a traceback (extend(cigar=False)) cannot be piled up")
        idx, rows, coff, cg = _hits_alns(self, self.score > 0)
        jobs = [tuple(int(x) for x in j) for j in jobs]
        rows["pattern"] = [jobs[i][0] for i in idx]
        rows["strand"] = [jobs[i][1] for i in idx]
        rows["tbeg"], rows["qbeg"] = self.tbeg[idx], self.qbeg[idx]
        return rows, coff, cg

    def pileup(self, index, patterns, jobs, window=None, add=False):
        """FMIndex.pileup of the jobs that aligned (score > 0)."""
        return index.pileup(patterns, self.alignments(jobs), window=window, add=add)


class MapResult:
    """Alignments of FMIndex.map, one per read: numpy arrays pattern, flags (MAP_REVERSE, MAP_UNMAPPED, MAP_TOO_LONG),
    record, offset (in the record), qbeg, qend (in the read as aligned: its reverse complement with MAP_REVERSE), tbeg,
    tend, score, sub, mapq, edits, diag (the diagonal of the extension job that won); cigar(i) as text, ops(i).  From
    FMIndex.map_chained also anchors(i): the winning chain as (qbeg, diag) pairs, diag[i] being the first one's."""

    def __init__(self, hits, offsets, cigars, anchor_offsets=None, anchor_rows=None):
        self.hits, self.offsets, self.cigars = hits, offsets, cigars
        self.anchor_offsets, self.anchor_rows = anchor_offsets, anchor_rows
        for name in _HIT_DTYPE.names:
            setattr(self, name, hits[name].copy())
        self.mapped = (self.flags & MAP_UNMAPPED) == 0
        self.strand = (self.flags & MAP_REVERSE).astype(np.uint8)

    def __len__(self):
        return len(self.hits)

    def ops(self, i):
        return self.cigars[int(self.offsets[i]):int(self.offsets[i + 1])]

    def cigar(self, i):
        return cigar_string(self.ops(i))

    def alignments(self, min_mapq=0):
        """The mapped hits of at least min_mapq as FMIndex.pileup takes them."""
        idx, rows, coff, cg = _hits_alns(self, self.mapped & (self.mapq >= min_mapq))
        rows["pattern"], rows["tbeg"], rows["qbeg"] = self.pattern[idx], self.tbeg[idx], self.qbeg[idx]
        rows["strand"] = self.strand[idx]
        return rows, coff, cg

    def pileup(self, index, patterns, min_mapq=0, window=None, add=False):
        """FMIndex.pileup of the mapped hits of at least min_mapq.  patterns: the reads that were mapped -- for map_pairs
        the mates interleaved (mate 1, mate 2 of pair 0, ...), the order of its hits."""
        return index.pileup(patterns, self.alignments(min_mapq), window=window, add=add)

    def anchors(self, i):
        if self.anchor_offsets is None:
            return None
        a = self.anchor_rows[int(self.anchor_offsets[i]):int(self.anchor_offsets[i + 1])]
        return [(int(q), int(d)) for q, d in zip(a["qbeg"], a["diag"])]


class SearchResult:
    """Hits of FMIndex.search: pattern i's hits are offsets[i] .. offsets[i + 1], ordered by (strand, mismatches, lo).
    ranges (H x 2) row intervals [lo, hi) as FMIndex.ranges gives them; mismatches and strands per hit."""

    def __init__(self, index, offsets, ranges, mismatches, strands):
        self.index, self.offsets, self.ranges, self.mismatches, self.strands = index, offsets, ranges, mismatches, strands

    def __len__(self):
        return len(self.offsets) - 1

    def hits(self, i):
        """(ranges, mismatches, strands) of pattern i"""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.ranges[a:b], self.mismatches[a:b], self.strands[a:b]

    def count(self):
        """occurrences per pattern: the sum of hi - lo over its hits (np.uint64)"""
        occ = (self.ranges[:, 1] - self.ranges[:, 0]).astype(np.uint64)
        cs = np.zeros(len(occ) + 1, dtype=np.uint64)
        np.cumsum(occ, out=cs[1:])
        return cs[self.offsets[1:].astype(np.int64)] - cs[self.offsets[:-1].astype(np.int64)]

    def locate(self, max_per_pattern=None):
        """FMIndex.locate_hits of this result"""
        return self.index.locate_hits(self, max_per_pattern)


class MemResult:
    """MEMs of FMIndex.mems: pattern i's MEMs are offsets[i] .. offsets[i + 1], ordered by (strand, qbeg).  spans (M x 2
    uint32) [qbeg, qend) in the pattern's coordinates (strand 1: the text reads the reverse complement of that span),
    ranges (M x 2 uint64) row intervals as FMIndex.ranges gives them, strands (uint8) per MEM."""

    def __init__(self, index, offsets, spans, ranges, strands):
        self.index, self.offsets, self.spans, self.ranges, self.strands = index, offsets, spans, ranges, strands

    def __len__(self):
        return len(self.offsets) - 1

    def hits(self, i):
        """(spans, ranges, strands) of pattern i"""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.spans[a:b], self.ranges[a:b], self.strands[a:b]

    def count(self):
        """occurrences per MEM: hi - lo (np.uint64)"""
        return (self.ranges[:, 1] - self.ranges[:, 0]).astype(np.uint64)

    def locate(self, max_per_mem=None):
        """global text positions of each MEM's occurrences (the first max_per_mem rows when capped), one uint64 array per
        MEM in row (suffix) order, through debwt_fm_locate"""
        r = np.ascontiguousarray(self.ranges, dtype=np.uint64)
        nm = len(r)
        cnt = r[:, 1] - r[:, 0]
        if max_per_mem is not None:
            cnt = np.minimum(cnt, np.uint64(max_per_mem))
        total = int(cnt.sum())
        offs = np.zeros(nm + 1, dtype=np.uint64)
        pos = np.empty(max(total, 1), dtype=np.uint64)
        if nm:
            self.index._chk(self.index._L.debwt_fm_locate(self.index._h, _p64(r), nm, int(max_per_mem or 0), _p64(offs),
                                                          _p64(pos), len(pos)))
        return [pos[int(offs[i]):int(offs[i + 1])] for i in range(nm)]


class KmerResult:
    """k-mer counts of FMIndex.kmer_counts: offsets (npat + 1 prefix sums of max(0, m - k + 1)) and counts (uint32);
    profile(i): the counts along pattern i."""

    def __init__(self, offsets, counts):
        self.offsets, self.counts = offsets, counts

    def __len__(self):
        return len(self.offsets) - 1

    def profile(self, i):
        return self.counts[int(self.offsets[i]):int(self.offsets[i + 1])]


class SpectrumResult:
    """Spectrum of FMIndex.spectrum: hist (uint64, hist[0] = 0, the last bin holds bins - 1 and above), distinct (the sum
    of hist), total (the sum of the multiplicities) and overflow_total (that sum over the last bin); threshold(): valley,
    peak and est_size (spectrum_threshold)."""

    def __init__(self, k, strands, hist, distinct, total, overflow_total):
        self.k, self.strands, self.hist = k, strands, hist
        self.distinct, self.total, self.overflow_total = distinct, total, overflow_total

    def threshold(self):
        return spectrum_threshold(self.hist, self.total)


class EsaResult:
    """The arrays FMIndex.esa left on the device.  lcp(lo, hi), sa(lo, hi), da(lo, hi): rows [lo, hi) (all rows by
    default) as uint32, uint64, uint32; sa and da raise DEBWT_ESTATE unless they were kept.  summary(): n, max, max_row,
    sum, capped, pos_prev, pos (the two places of the longest repeat), cap.  profile(kmax): distinct[k - 1] = the number
    of distinct k-mers inside records, k = 1 .. kmax <= min(cap, 4096).  The arrays belong to the index: the next esa()
    replaces them and release() frees them, after which every method raises DEBWT_ESTATE.  repeats(): the maximal
    repeats, the supermaximal repeats or all intervals of the LCP array (Definition 11), from the LCP array alone.
    records_build() (needs da) adds the prefix array of Definition 12; record_counts(), repeats_by_record() and mums()
    then answer in how many distinct records a row range or a repeat occurs."""

    _ARRAYS = {"lcp": (0, np.uint32), "sa": (1, np.uint64), "da": (2, np.uint32)}

    def __init__(self, index):
        self._x = index

    def _fetch(self, name, lo, hi):
        which, dtype = self._ARRAYS[name]
        x = self._x
        lo = int(lo)
        hi = x.info()["n"] if hi is None else int(hi)
        if hi < lo:
            raise ValueError("hi must not be below lo")
        out = np.zeros(hi - lo, dtype=dtype)
        x._chk(x._L.debwt_fm_esa_fetch(x._h, which, lo, hi - lo, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def lcp(self, lo=0, hi=None):
        return self._fetch("lcp", lo, hi)

    def sa(self, lo=0, hi=None):
        return self._fetch("sa", lo, hi)

    def da(self, lo=0, hi=None):
        return self._fetch("da", lo, hi)

    def summary(self):
        out = _lib.DebwtFmEsaSummary()
        self._x._chk(self._x._L.debwt_fm_esa_summary_get(self._x._h, ctypes.byref(out)))
        return out.as_dict()

    def profile(self, kmax):
        out = np.zeros(max(int(kmax), 1), dtype=np.uint64)
        self._x._chk(self._x._L.debwt_fm_esa_profile(self._x._h, int(kmax), _p64(out)))
        return out[:int(kmax)]

    def repeats(self, min_len=20, min_occ=2, max_occ=None, kind="maximal"):
        """The repeats of the collection (debwt_fm_repeats): the intervals of the LCP array with len >= min_len and
        min_occ <= count <= max_occ (None: no bound) of kind "maximal", "supermaximal" or "intervals" (every interval, left-
        diverse or not), ascending by representative row.  A structured array (REPEAT_DTYPE): row_lo and count name the
        rows [row_lo, row_lo + count) -- sa(row_lo, row_lo + count) are the occurrences when sa was kept --, left the
        occurrences behind A, C, G, T and at a record's start, len the length, flags REPEAT_IS_MAXIMAL and
        REPEAT_IS_SUPERMAXIMAL.  With a capped build the intervals of the capped value are left out and counted in
        repeat_stats()["capped_intervals"]."""
        if kind not in REPEAT_KINDS:
            raise ValueError('kind must be "maximal", "supermaximal" or "intervals"')
        x = self._x
        opts = _lib.DebwtFmRepeatOpts(int(min_len), REPEAT_KINDS[kind], int(min_occ), int(max_occ or 0))
        n = ctypes.c_uint64(0)
        rc = x._L.debwt_fm_repeats(x._h, ctypes.byref(opts), None, 0, ctypes.byref(n))     # the sizing call: ERANGE names the count
        if rc != -5:
            x._chk(rc)
        out = np.zeros(n.value, dtype=REPEAT_DTYPE)
        if n.value:
            x._chk(x._L.debwt_fm_repeats(x._h, ctypes.byref(opts), out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return out[:n.value]

    def records_build(self):
        """The prefix array of Definition 12 on the device (debwt_fm_records_build): after it record_counts,
        repeats_by_record and mums answer in how many distinct records an interval occurs.  Needs esa(da=True); kept with
        the arrays, counted in info()["device_bytes"], released with them."""
        self._x._chk(self._x._L.debwt_fm_records_build(self._x._h))
        return self

    def dup_prefix(self, lo=0, hi=None):
        """P[lo .. hi) of Definition 12 as uint64 (all rows by default)."""
        x = self._x
        lo = int(lo)
        hi = x.info()["n"] if hi is None else int(hi)
        if hi < lo:
            raise ValueError("hi must not be below lo")
        out = np.zeros(hi - lo, dtype=np.uint64)
        x._chk(x._L.debwt_fm_records_fetch(x._h, lo, hi - lo, _p64(out)))
        return out

    def record_counts(self, ranges):
        """The distinct records of each row range [lo, hi) (debwt_fm_record_counts), uint64: ranges is (k, 2), as
        FMIndex.ranges answers.  Exact for closed ranges (every LCP interval, every pattern no longer than the cap of the
        build); for other ranges the value of the formula of Definition 12, which is no record count."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
        out = np.zeros(len(r), dtype=np.uint64)
        if len(r):
            self._x._chk(self._x._L.debwt_fm_record_counts(self._x._h, _p64(r), len(r), _p64(out)))
        return out

    def repeats_by_record(self, min_len=20, min_occ=2, max_occ=None, kind="maximal", min_records=1, max_records=None,
                          unique=False):
        """repeats() filtered by the distinct records of every interval (debwt_fm_repeats_records): min_records <= records
        <= max_records (None: no bound), and count == records with unique (no record holds the string twice).  Returns
        (the REPEAT_DTYPE array, the records of each entry as uint32).  Needs records_build()."""
        if kind not in REPEAT_KINDS:
            raise ValueError('kind must be "maximal", "supermaximal" or "intervals"')
        x = self._x
        opts = _lib.DebwtFmRepeatOpts(int(min_len), REPEAT_KINDS[kind], int(min_occ), int(max_occ or 0))
        flt = _lib.DebwtFmRecordFilter(int(min_records), int(max_records or 0), RECORDS_UNIQUE if unique else 0, 0)
        n = ctypes.c_uint64(0)
        rc = x._L.debwt_fm_repeats_records(x._h, ctypes.byref(opts), ctypes.byref(flt), None, None, 0, ctypes.byref(n))
        if rc != -5:                                           # the sizing call: ERANGE names the count
            x._chk(rc)
        out = np.zeros(n.value, dtype=REPEAT_DTYPE)
        recs = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            x._chk(x._L.debwt_fm_repeats_records(x._h, ctypes.byref(opts), ctypes.byref(flt), out.ctypes.data_as(ctypes.c_void_p),
                                                 recs.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return out[:n.value], recs[:n.value]

    def mums(self, min_len=20, min_records=None):
        """The multi-MUMs of the collection (Definition 12): maximal repeats of len >= min_len that occur once in each of
        at least min_records records and nowhere else; min_records defaults to all records of the index.  Returns what
        repeats_by_record returns."""
        q = self._x.info()["nrec"] if min_records is None else int(min_records)
        return self.repeats_by_record(min_len=min_len, min_occ=max(q, 2), kind="maximal", min_records=q, unique=True)

    def cdbg(self, k, strands="forward"):
        """The compacted de Bruijn graph of the collection's k-mers.  strands="forward": Definition 13 (debwt_fm_cdbg), a
        k-mer and its reverse complement are two nodes.  strands="both": Definition 14 (debwt_fm_cdbg_both), bidirected
        unitigs over canonical k-mers, k odd; an edge end is 2 * unitig + orientation.  Needs esa(sa=True, da=True) with
        max_lcp 0 or at least k + 1.  Returns a CdbgResult."""
        if strands not in ("forward", "both"):
            raise ValueError('strands must be "forward" or "both"')
        x = self._x
        call = x._L.debwt_fm_cdbg_both if strands == "both" else x._L.debwt_fm_cdbg
        sz = _lib.DebwtFmCdbgSizes()
        rc = call(x._h, int(k), 0, None, 0, None, 0, None, 0, ctypes.byref(sz))   # the sizing call: ERANGE names the sizes
        if rc != -5:
            x._chk(rc)
        un = np.zeros(sz.unitigs, dtype=UNITIG_DTYPE)
        seq = np.zeros(sz.seq_bytes, dtype=np.uint8)
        ed = np.zeros(sz.edges, dtype=CDBG_EDGE_DTYPE)
        if sz.unitigs:
            x._chk(call(x._h, int(k), 0, un.ctypes.data_as(ctypes.c_void_p), len(un),
                        seq.ctypes.data_as(ctypes.c_void_p), len(seq), ed.ctypes.data_as(ctypes.c_void_p), len(ed),
                        ctypes.byref(sz)))
        return CdbgResult(int(k), un[:sz.unitigs], seq[:sz.seq_bytes], ed[:sz.edges], strands)

    def release(self):
        self._x._chk(self._x._L.debwt_fm_esa_release(self._x._h))


class CdbgResult:
    """What EsaResult.cdbg returns: unitigs (UNITIG_DTYPE: row_lo, seq_offset, kmer_count, nodes, flags with CDBG_CIRCULAR),
    numbered by the string order of their first k-mers; seq, the unitig strings as ASCII bytes packed in that order; edges
    (CDBG_EDGE_DTYPE: from, to in unitig numbers, ascending).  strings() cuts seq into one str per unitig.  With strands =
    "both" the unitigs are numbered by the row of w* (Definition 14) and an edge end is 2 * unitig + orientation, orientation 1
    for the unitig read reverse-complemented."""

    def __init__(self, k, unitigs, seq, edges, strands="forward"):
        self.k, self.unitigs, self.seq, self.edges, self.strands = k, unitigs, seq, edges, strands

    def strings(self):
        s = self.seq.tobytes().decode()
        return [s[int(u["seq_offset"]):int(u["seq_offset"]) + int(u["nodes"]) + self.k - 1] for u in self.unitigs]


class OverlapResult:
    """Overlaps of FMIndex.overlaps: pattern i's hits are offsets[i] .. offsets[i + 1], ordered by (strand, length
    descending, record).  all_hits: structured array with record, length, strand (0 forward, 1 reverse complement) and
    flags (OVERLAP_CONTAINS: the record is as long as the overlap; OVERLAP_WHOLE: the pattern is; from overlaps_mm also the
    hit's mismatches in bits 8-15, see mismatches())."""

    def __init__(self, index, offsets, hits):
        self.index, self.offsets, self.all_hits = index, offsets, hits

    def __len__(self):
        return len(self.offsets) - 1

    def hits(self, i):
        """structured array (record, length, strand, flags) of pattern i"""
        return self.all_hits[int(self.offsets[i]):int(self.offsets[i + 1])]

    def count(self):
        """hits per pattern (np.uint64)"""
        return self.offsets[1:] - self.offsets[:-1]

    def mismatches(self):
        """mismatches per hit (np.uint8, flags bits 8-15): zeros for a result of FMIndex.overlaps"""
        return ((self.all_hits["flags"] >> 8) & 0xFF).astype(np.uint8)


class _GraphArrays:
    """what GraphResult and BiGraphResult share: the three arrays of a string graph and the out-list of a node"""

    def __init__(self, index, state, offsets, edges, reduced):
        self.index, self.state, self.offsets, self.edges, self.reduced = index, state, offsets, edges, reduced

    def __len__(self):
        return len(self.state)

    def out(self, i):
        """structured array (record, length) of the out-edges of record i (GraphResult) or node i (BiGraphResult)"""
        return self.edges[int(self.offsets[i]):int(self.offsets[i + 1])]

    def clean(self, max_tip=4, max_bubble=16, max_rounds=8):
        """The graph with its tips clipped and its bubbles popped (graph_clean(), on the graph's index; mirrored for a
        BiGraphResult): a new result of the same class whose state holds NODE_CLIPPED and NODE_POPPED for the nodes
        removed and whose edges are those between the nodes left, in their order.  unitigs() and sequences() work on it
        as before.  ValueError for a graph that is not reduced."""
        if not self.reduced:
            raise ValueError("clean() needs the irreducible graph (reduce=True)")
        state, keep = graph_clean(self.index, self.state, self.offsets, self.edges, max_tip, max_bubble, max_rounds,
                                  mirrored=isinstance(self, BiGraphResult))
        offs, edges = edges_compact(self.offsets, self.edges, keep)
        return type(self)(self.index, state, offs, edges, True)


class GraphResult(_GraphArrays):
    """String graph of FMIndex.string_graph.  state: per record NODE_KEPT, NODE_DUPLICATE or NODE_CONTAINED; record i's
    out-edges are edges[offsets[i] .. offsets[i + 1]), a structured array of (record, length) ordered by (length descending,
    record): record i's last `length` bases are the first `length` of `record`.  reduced: the edges are those of the
    irreducible graph, which unitigs() needs."""

    def unitigs(self):
        """(offsets, members, circular) of the unbranched paths, see unitigs()"""
        return unitigs(self.state, self.offsets, self.edges)

    def sequences(self, index=None):
        """The unitigs' sequences as a list of str, through FMIndex.extract of `index` (default: the graph's own): every
        member but the last gives its first |S| - L_next bases, and the last of a circular unitig is cut by its overlap
        with the first."""
        index = self.index if index is None else index
        uoff, mem, circ = self.unitigs()
        starts = np.append(index.record_starts(), np.uint64(index.n))
        jobs = []
        for u in range(len(circ)):
            m = [int(x) for x in mem[int(uoff[u]):int(uoff[u + 1])]]
            for x, v in enumerate(m):
                length = int(starts[v + 1]) - 1 - int(starts[v])
                if x + 1 < len(m) or circ[u]:
                    length -= int(self.out(v)["length"][0])    # a link's source has one out-edge
                jobs.append((v, 0, length))
        parts = index.extract(jobs)
        return [b"".join(parts[int(uoff[u]):int(uoff[u + 1])]).decode() for u in range(len(circ))]


def edges_reduce(index, reclen, offsets, edges):
    """Transitive reduction of any edge list on the index's GPU (debwt_fm_edges_reduce).  reclen: the nodes' lengths;
    node i's edges are edges[offsets[i] .. offsets[i + 1]), (record, length) with lengths descending, one length's records
    in any order.  Returns keep, one np.uint8 per edge: 0 for an edge (i -> k, L) that some (i -> j, L_ij > L) and (j -> k,
    reclen[j] - L_ij + L) explain.  A list out of that order, a repeated or out-of-range target, a self edge or a length
    that covers a node raises DebwtError (DEBWT_EINVAL)."""
    reclen = np.ascontiguousarray(reclen, dtype=np.uint64)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    e = np.ascontiguousarray(np.asarray(edges, dtype=_EDGE_DTYPE))
    if len(offs) != len(reclen) + 1 or int(offs.max()) > len(e):
        raise ValueError("offsets fit neither the nodes nor the edges")
    keep = np.zeros(max(len(e), 1), dtype=np.uint8)
    index._chk(index._L.debwt_fm_edges_reduce(index._h, _p64(reclen) if len(reclen) else None, len(reclen), _p64(offs),
                                              e.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmEdge)),
                                              keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
    return keep[:len(e)]


def graph_clean(index, state, offsets, edges, max_tip=4, max_bubble=16, max_rounds=8, mirrored=False):
    """Tips and bubbles of any graph on the index's GPU (debwt_fm_graph_clean, definition 6 of debwt_hip.h).  state: one
    byte per node, 0 for a node that takes part; node i's edges are edges[offsets[i] .. offsets[i + 1]).  A dead-end chain of
    at most max_tip nodes at a junction that has another way on is clipped (NODE_CLIPPED); of the unbranched chains of at
    most max_bubble nodes that lead from one junction to one node, all but the longest (then the one with the lowest node)
    are popped (NODE_POPPED); rounds of both repeat until one removes nothing or max_rounds have run.  mirrored: the node
    ids are 2r + o of a graph over both strands, and a bubble gets the same verdict from both ends.  Returns (state_out,
    edge_keep), one np.uint8 per node and per edge.  An edge at a node whose state is not 0, a target out of range, no
    phase to run (max_tip == max_bubble == 0) or max_rounds == 0 raises DebwtError (DEBWT_EINVAL)."""
    state = np.ascontiguousarray(state, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    e = np.ascontiguousarray(np.asarray(edges, dtype=_EDGE_DTYPE))
    nn = len(state)
    if len(offs) != nn + 1 or int(offs.max()) > len(e):
        raise ValueError("offsets fit neither the nodes nor the edges")
    opts = _lib.DebwtFmCleanOpts(int(max_tip), int(max_bubble), int(max_rounds), CLEAN_MIRRORED if mirrored else 0)
    out = np.zeros(max(nn, 1), dtype=np.uint8)
    keep = np.zeros(max(len(e), 1), dtype=np.uint8)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    index._chk(index._L.debwt_fm_graph_clean(index._h, state.ctypes.data_as(u8p) if nn else None, _p64(offs),
                                             e.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmEdge)) if len(e) else None, nn,
                                             ctypes.byref(opts), out.ctypes.data_as(u8p), keep.ctypes.data_as(u8p)))
    return out[:nn], keep[:len(e)]


def edges_compact(offsets, edges, keep):
    """(offsets_out, edges_out): the edges with keep != 0, in their order, on the host (debwt_fm_edges_compact)"""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    e = np.ascontiguousarray(np.asarray(edges, dtype=_EDGE_DTYPE))
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    if len(offs) < 1 or int(offs.max()) > len(e) or len(keep) != len(e):
        raise ValueError("offsets and keep do not fit the edges")
    nn = len(offs) - 1
    out_offs = np.zeros(nn + 1, dtype=np.uint64)
    out = np.zeros(max(len(e), 1), dtype=_EDGE_DTYPE)
    edgep = ctypes.POINTER(_lib.DebwtFmEdge)
    rc = _lib.lib().debwt_fm_edges_compact(_p64(offs), e.ctypes.data_as(edgep) if len(e) else None,
                                           keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if len(e) else None, nn,
                                           _p64(out_offs), out.ctypes.data_as(edgep))
    if rc:
        raise DebwtError(rc)
    return out_offs, out[:int(out_offs[nn])].copy()


def unitigs(state, offsets, edges):
    """The unbranched paths of a graph over the kept nodes (state 0) on the host (debwt_fm_unitigs, no GPU).  u -> w is a
    link iff w is u's only successor, u is w's only predecessor and w != u; a unitig is a maximal chain of links, a cycle
    of links starts at its lowest node.  Returns (offsets, members, circular): unitig t's nodes are members[offsets[t] ..
    offsets[t + 1]) in path order, unitigs by ascending first node, circular one np.uint8 each."""
    return _unitig_call(_lib.lib().debwt_fm_unitigs, state, offsets, edges)


def _unitig_call(fn, state, offsets, edges):
    """(offsets, members, circular) of debwt_fm_unitigs or debwt_fm_unitigs_both"""
    state = np.ascontiguousarray(state, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    e = np.ascontiguousarray(np.asarray(edges, dtype=_EDGE_DTYPE))
    nn = len(state)
    if len(offs) != nn + 1 or int(offs.max()) > len(e):
        raise ValueError("offsets fit neither the nodes nor the edges")
    uoff = np.zeros(nn + 1, dtype=np.uint64)
    mem = np.zeros(max(nn, 1), dtype=np.uint32)
    circ = np.zeros(max(nn, 1), dtype=np.uint8)
    nu = ctypes.c_uint64(0)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    rc = fn(state.ctypes.data_as(u8p) if nn else None, _p64(offs), e.ctypes.data_as(ctypes.POINTER(_lib.DebwtFmEdge)) if len(e) else None,
            nn, _p64(uoff), mem.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), circ.ctypes.data_as(u8p), ctypes.byref(nu))
    if rc:
        raise DebwtError(rc)
    k = int(nu.value)
    return uoff[:k + 1].copy(), mem[:int(uoff[k])].copy(), circ[:k].copy()


def unitigs_both(state, offsets, edges):
    """The oriented unitigs of a graph over both strands on the host (debwt_fm_unitigs_both, no GPU): nodes 2r + o; a link
    is one of unitigs() that does not lead to its source's mirror (v ^ 1) and touches no self-rc read (state[2r] == 0,
    state[2r + 1] == 1).  Of a unitig and its mirror the one with the lower first member is returned, so every kept read
    is in exactly one, in one orientation.  Returns (offsets, members, circular) as unitigs() does."""
    return _unitig_call(_lib.lib().debwt_fm_unitigs_both, state, offsets, edges)


_RC = bytes.maketrans(b"ACGT", b"TGCA")


class BiGraphResult(_GraphArrays):
    """String graph over both strands of FMIndex.string_graph_both.  Node 2r + o is read r as it is (o = 0) or its reverse
    complement (o = 1).  state: per node NODE_KEPT, NODE_DUPLICATE or NODE_CONTAINED (the second node of a self-rc read is
    a duplicate of the first); node v's out-edges are edges[offsets[v] .. offsets[v + 1]), (record, length) with record
    the target node, ordered by (length descending, record).  reduced: the irreducible graph, which unitigs() needs."""

    def unitigs(self):
        """(offsets, members, circular) of the oriented unitigs, see unitigs_both()"""
        return unitigs_both(self.state, self.offsets, self.edges)

    def sequences(self, index=None):
        """The unitigs' sequences as a list of str, through FMIndex.extract of `index` (default: the graph's own) and a
        reverse complement on the host for the members of orientation 1: every member but the last gives the first
        |S| - L_next bases of its oriented string, and the last of a circular unitig is cut by its overlap with the first."""
        index = self.index if index is None else index
        uoff, mem, circ = self.unitigs()
        starts = np.append(index.record_starts(), np.uint64(index.n))
        jobs = []
        for u in range(len(circ)):
            m = [int(x) for x in mem[int(uoff[u]):int(uoff[u + 1])]]
            for x, v in enumerate(m):
                r = v >> 1
                full = int(starts[r + 1]) - 1 - int(starts[r])
                cut = int(self.out(v)["length"][0]) if x + 1 < len(m) or circ[u] else 0   # a link's source has one out-edge
                jobs.append((r, cut, full - cut) if v & 1 else (r, 0, full - cut))
        parts = index.extract(jobs)
        parts = [p.translate(_RC)[::-1] if int(v) & 1 else p for p, v in zip(parts, mem)]
        return [b"".join(parts[int(uoff[u]):int(uoff[u + 1])]).decode() for u in range(len(circ))]


class MultiDeBWT:
    """One BWT over several GPUs from one process (debwt_multi_*): one host thread per GPU, peer-to-peer exchanges.
    devices: HIP ordinals of the shards (may repeat: several shards on one GPU)."""

    def __init__(self, devices, k=32, tune=0):
        self._L = _lib.lib()
        cfg = _lib.DebwtConfig(k=k, device=0, sort_algo=0, reserved=tune)
        dv = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = self._L.debwt_multi_create(ctypes.byref(cfg), dv, len(devices), ctypes.byref(h))
        if rc:
            raise DebwtError(rc)
        self._h, self.n, self.nrec, self._keep = h, 0, 0, None

    def close(self):
        if getattr(self, "_h", None):
            self._L.debwt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc:
            raise DebwtError(rc, self._L.debwt_multi_last_error(self._h).decode())

    def _shard_ctx(self, shard):
        return ctypes.c_void_p(self._L.debwt_multi_shard(self._h, shard))

    def load_packed(self, words, n, sep):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        sep = np.ascontiguousarray(sep, dtype=np.uint64)
        self._keep = (words, sep)
        self._chk(self._L.debwt_multi_load_text(self._h, _p64(words), n, _p64(sep), len(sep)))
        self.n, self.nrec = n, len(sep)

    def load_records(self, records):
        self.load_packed(*pack_records(records))

    def set_key_mode(self, mode):
        """"exchange", "rescan" or "auto" (the library's cost model decides): how the keys reach their shards."""
        self._chk(self._L.debwt_multi_set_key_mode(self._h, {"exchange": 0, "rescan": 1, "auto": -1}[mode]))

    def set_exchange(self, backend):
        """"peer" (device-to-device copies, the default) or "rccl" (grouped ncclSend / ncclRecv; one distinct GPU per shard)."""
        self._chk(self._L.debwt_multi_set_exchange(self._h, {"peer": 0, "rccl": 1}[backend]))

    def build(self):
        self._chk(self._L.debwt_multi_build(self._h))

    def fetch(self):
        words = np.empty((self.n + 31) // 32, dtype=np.uint64)
        hrows = np.empty(max(self.nrec - 1, 1), dtype=np.uint64)
        drow = np.empty(1, dtype=np.uint64)
        self._chk(self._L.debwt_multi_fetch_bwt(self._h, _p64(words), _p64(hrows), _p64(drow)))
        return words, hrows[:self.nrec - 1], int(drow[0])

    def stats(self):
        ms, s0 = _lib.DebwtMultiStats(), _lib.DebwtStats()
        self._chk(self._L.debwt_multi_get_stats(self._h, ctypes.byref(ms), ctypes.byref(s0)))
        return ms.as_dict(), s0.as_dict()

    def set_serial(self, on=True):
        """The shards of a build take turns between the barriers, one on its GPU at a time (debwt_multi_set_serial): how the
        per-shard times of N = 2, 4, 8 are measured on a box with one GPU."""
        self._chk(self._L.debwt_multi_set_serial(self._h, 1 if on else 0))

    def shard_report(self, shard):
        """What shard `shard` did in the last build: wall ms per step (by name), bytes in/out per exchange, its sizes, and the
        device-side stage times and counters of its context."""
        rep = _lib.DebwtShardReport()
        self._chk(self._L.debwt_multi_get_shard_report(self._h, int(shard), ctypes.byref(rep)))
        names = [self._L.debwt_multi_step_name(i).decode() for i in range(_lib.MULTI_STEPS)]
        xn = ("keys", "facts", "sp", "blue", "rows")
        st = _lib.DebwtStats()
        self._L.debwt_get_stats(self._shard_ctx(shard), ctypes.byref(st))
        return {"shard": int(shard), "bins": [int(rep.bin_lo), int(rep.bin_hi)], "keys": int(rep.keys),
                "key_ranges": int(rep.key_ranges), "blocks": int(rep.blocks), "blue_rows": int(rep.blue_rows), "rows": int(rep.rows),
                "ms": {nm: round(float(rep.ms[i]), 3) for i, nm in enumerate(names) if rep.ms[i] > 0},
                "bytes_in": {x: int(rep.bytes_in[i]) for i, x in enumerate(xn)},
                "bytes_out": {x: int(rep.bytes_out[i]) for i, x in enumerate(xn)},
                "ctx": st.as_dict()}

    def verify_device(self):
        rep = _lib.DebwtVerifyReport()
        self._chk(self._L.debwt_multi_verify(self._h, ctypes.byref(rep)))
        return rep.as_dict()


def verify_inverse(words, n, hash_rows, dollar_row):
    """Inverse BWT by LF walk on the host (the job of the reference's dead LFsearch path)."""
    L = _lib.lib()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    hr = np.ascontiguousarray(hash_rows, dtype=np.uint64)
    nrec = len(hr) + 1
    if len(hr) == 0:
        hr = np.zeros(1, dtype=np.uint64)
    out = np.empty(n, dtype=np.uint8)
    rc = L.debwt_verify_inverse(_p64(words), n, _p64(hr), nrec, int(dollar_row),
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return rc, out


def write_outputs(path, words, hash_rows, dollar_row):
    """OUT, OUT.#, OUT.$ exactly as src/insertCase3.c:115-131 writes them."""
    np.ascontiguousarray(words, dtype=np.uint64).tofile(path)
    np.ascontiguousarray(hash_rows, dtype=np.uint64).tofile(path + ".#")
    np.array([dollar_row], dtype=np.uint64).tofile(path + ".$")


FASTA_IUPAC_RANDOM = 1


def fasta_text_bound(path):
    """Upper bound of the text length the file can hold, from its size and framing alone (0: not known); debwt_fasta_text_bound."""
    return int(_lib.lib().debwt_fasta_text_bound(str(path).encode()))


def pack_fasta(path, threads=8, iupac_seed=None):
    """Host-only: (words, n, sep, seconds_read, seconds_pack) of a FASTA file in the reference's 2-bit layout."""
    L = _lib.lib()
    pt = _lib.DebwtPackedText()
    err = ctypes.create_string_buffer(256)
    if iupac_seed is None:
        rc = L.debwt_pack_fasta(str(path).encode(), int(threads), ctypes.byref(pt), err, 256)
    else:
        rc = L.debwt_pack_fasta_opts(str(path).encode(), int(threads), FASTA_IUPAC_RANDOM, int(iupac_seed), ctypes.byref(pt), err, 256)
    if rc:
        raise DebwtError(rc, err.value.decode())
    try:
        words = np.ctypeslib.as_array(pt.words, shape=(pt.nwords,)).copy()
        sep = np.ctypeslib.as_array(pt.sep, shape=(pt.nrec,)).copy()
        return words, int(pt.n), sep, pt.seconds_read, pt.seconds_pack
    finally:
        L.debwt_free_packed(ctypes.byref(pt))
