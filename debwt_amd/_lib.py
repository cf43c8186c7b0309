"""ctypes loader of libdebwt_hip.so (include/debwt_hip.h).  There is no CPU fallback: if the HIP
library is missing or cannot be loaded, every entry point raises."""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEBWT_HIP_LIB", os.path.join(_HERE, "libdebwt_hip.so"))   # override: kernel experiments only
_lib = None


class DebwtConfig(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int), ("device", ctypes.c_int), ("sort_algo", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class DebwtPackedText(ctypes.Structure):
    _fields_ = [("words", ctypes.POINTER(ctypes.c_uint64)), ("nwords", ctypes.c_uint64), ("n", ctypes.c_uint64),
                ("sep", ctypes.POINTER(ctypes.c_uint64)), ("nrec", ctypes.c_uint64),
                ("seconds_read", ctypes.c_double), ("seconds_pack", ctypes.c_double)]


class DebwtStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in (
        "n", "nrec", "red_capacity", "blue_capacity", "blue_bound_num", "case3num", "sp_len",
        "special_branch_num", "n_main", "distinct_keys", "blue_large_blocks", "blue_max_block")] +
        [(n, ctypes.c_float) for n in (
            "ms_extract", "ms_sort", "ms_classify", "ms_sp", "ms_blue", "ms_assemble", "ms_total",
            "ms_host_special")] +
        [("radix_pass_launches", ctypes.c_uint32), ("radix_pass_ms", ctypes.c_float),
         ("radix_pass_keys", ctypes.c_uint64), ("special_path", ctypes.c_uint32), ("special_threads", ctypes.c_uint32),
         ("sort_unfit_stretches", ctypes.c_uint64), ("sort_unfit_network", ctypes.c_uint64),
         ("sort_over_stretches", ctypes.c_uint64), ("sort_bucket_passes", ctypes.c_uint64)])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtVerifyReport(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("segments", "steps", "mismatches", "broken_links", "search_failures",
                                                "search_steps")] +
                [(n, ctypes.c_float) for n in ("ms_index", "ms_search", "ms_walk")] + [("ok", ctypes.c_int)])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


MULTI_STEPS = 24


class DebwtShardReport(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_float * MULTI_STEPS), ("bytes_in", ctypes.c_uint64 * 5), ("bytes_out", ctypes.c_uint64 * 5),
                ("keys", ctypes.c_uint64), ("key_ranges", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("blue_rows", ctypes.c_uint64), ("rows", ctypes.c_uint64), ("bin_lo", ctypes.c_uint32), ("bin_hi", ctypes.c_uint32)]


class DebwtFmInfo(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("n", "nrec", "sa_sample", "samples", "device_bytes")] +
                [("ms_rank", ctypes.c_float), ("ms_samples", ctypes.c_float), ("census", ctypes.c_uint64 * 4)])

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["census"] = [int(x) for x in self.census]
        return d


class DebwtFmSearchStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("patterns", "batches", "launches", "retries", "hits", "steps", "line_reads",
                                                 "scratch_bytes")] +
                [("items", ctypes.c_uint64 * 5), ("ms_kernel", ctypes.c_float), ("ms_wall", ctypes.c_float)])

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["items"] = [int(x) for x in self.items]
        return d


class DebwtFmMemsStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("patterns", "batches", "launches", "mems", "steps", "line_reads", "wave_steps",
                                                 "scratch_bytes")] +
                [("ms_kernel", ctypes.c_float), ("ms_wall", ctypes.c_float)])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmOverlapsStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("patterns", "batches", "launches", "runs", "hits", "steps", "line_reads",
                                                 "wave_steps", "scratch_bytes")] +
                [("ms_kernel", ctypes.c_float), ("ms_wall", ctypes.c_float)])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmOverlapsMmStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("patterns", "batches", "launches", "retries", "runs", "hits", "steps",
                                                 "line_reads", "wave_steps", "scratch_bytes")] +
                [("items", ctypes.c_uint64 * 5), ("ms_kernel", ctypes.c_float), ("ms_wall", ctypes.c_float)])

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["items"] = [int(x) for x in self.items]
        return d


class DebwtFmExtractStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("jobs", "batches", "launches", "segments", "bases", "steps", "wave_steps",
                                                 "line_reads", "anchor_bytes")] +
                [(n, ctypes.c_float) for n in ("ms_anchors", "ms_kernel", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmKmerStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("patterns", "batches", "launches", "kmers", "steps", "line_reads", "wave_steps",
                                                 "table_starts", "scratch_bytes")] +
                [("table_q", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] +
                [(n, ctypes.c_float) for n in ("ms_table", "ms_kernel", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class DebwtFmSpectrumTotals(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("distinct", "total", "overflow_total")]


class DebwtFmSpectrumSummary(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("valley", "peak", "est_size")]


class DebwtFmSpectrumStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("chunks", "launches", "levels", "expanded", "leaves", "lookups", "steps",
                                                 "line_reads", "wave_steps", "scratch_bytes", "items_limit")] +
                [("level_intervals", ctypes.c_uint64 * 33), ("table_q", ctypes.c_uint32), ("reserved", ctypes.c_uint32)] +
                [(n, ctypes.c_float) for n in ("ms_table", "ms_kernel", "ms_wall")])

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("reserved", "level_intervals")}
        d["level_intervals"] = [int(x) for x in self.level_intervals]
        return d


class DebwtFmEsaSummary(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n", "max", "max_row", "sum", "capped", "pos_prev", "pos", "cap")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class DebwtFmEsaStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("walk_items", "walk_steps", "walk_wave_steps", "chunks", "chunk_len",
                                                 "symbols_compared", "plcp_wave_steps", "build_bytes", "kept_bytes")] +
                [(n, ctypes.c_float) for n in ("ms_walk", "ms_scatter", "ms_plcp", "ms_rows", "ms_text", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmRepeatOpts(ctypes.Structure):
    _fields_ = [("min_len", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("min_occ", ctypes.c_uint64), ("max_occ", ctypes.c_uint64)]


class DebwtFmRepeatStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("rows", "searched", "representatives", "intervals", "maximal", "supermaximal",
                                                 "capped_intervals", "reported", "longest_len", "longest_row_lo", "levels",
                                                 "fanout", "tree_bytes", "scratch_bytes", "search_steps", "wave_steps",
                                                 "rank_lines")] +
                [(n, ctypes.c_float) for n in ("ms_tree", "ms_search", "ms_write", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmRecordFilter(ctypes.Structure):
    _fields_ = [("min_records", ctypes.c_uint64), ("max_records", ctypes.c_uint64), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class DebwtFmRecordsStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("rows", "pairs", "records_present", "sort_passes", "levels", "fanout",
                                                 "rmq_steps", "wave_steps", "build_bytes", "kept_bytes")] +
                [(n, ctypes.c_float) for n in ("ms_sort", "ms_tree", "ms_pairs", "ms_scan", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmCdbgSizes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("unitigs", "seq_bytes", "edges")]


class DebwtFmCdbgStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("nodes", "edge_strings", "unitigs", "circular", "links", "edges", "longest_nodes",
                                                 "seq_bytes", "jump_rounds", "jump_steps", "jump_wave_steps", "rank_lines",
                                                 "scratch_bytes")] +
                [(n, ctypes.c_float) for n in ("ms_nodes", "ms_links", "ms_rank", "ms_write", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmCdbgBothStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("nodes", "edge_strings", "unitigs", "circular", "links", "edges", "longest_nodes",
                                                 "seq_bytes", "present", "mated", "hairpins", "jump_rounds", "jump_steps",
                                                 "jump_wave_steps", "rank_lines", "mate_steps", "edge_keys", "scratch_bytes")] +
                [(n, ctypes.c_float) for n in ("ms_nodes", "ms_mates", "ms_links", "ms_rank", "ms_write", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


CORRECT_MAX_ROUNDS = 16


class DebwtFmCorrectStats(ctypes.Structure):
    _fields_ = ([("kmers", DebwtFmKmerStats)] +
                [(n, ctypes.c_uint64) for n in ("rounds", "trials", "fixes", "reads_short", "reads_clean", "reads_fixed",
                                                 "reads_weak")] +
                [("active", ctypes.c_uint64 * CORRECT_MAX_ROUNDS), ("ms_round", ctypes.c_float * CORRECT_MAX_ROUNDS)])

    def as_dict(self):
        d = self.kmers.as_dict()
        d.update({n: getattr(self, n) for n, _ in self._fields_[1:8]})
        d["active"] = [int(x) for x in self.active]
        d["ms_round"] = [float(x) for x in self.ms_round]
        return d


class DebwtFmTrial(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("run_a", "run_b", "pos", "window", "kind")]


class DebwtFmCorrectOpts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("k", "min_count", "max_rounds", "flags")]


class DebwtFmCorrectInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("flags", "fixes", "weak_before", "weak_after")]


class DebwtFmExtractJob(ctypes.Structure):
    _fields_ = [("record", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("offset", ctypes.c_uint64),
                ("length", ctypes.c_uint64)]


class DebwtFmOverlap(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("record", "length", "strand", "flags")]


class DebwtFmEdge(ctypes.Structure):
    _fields_ = [("record", ctypes.c_uint32), ("length", ctypes.c_uint32)]


class DebwtFmGraphStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("records", "kept", "duplicates", "contained", "hits", "edges", "reducible",
                                                 "lookups", "launches", "scratch_bytes", "edge_bytes")] +
                [(n, ctypes.c_float) for n in ("ms_walk", "ms_build", "ms_reduce", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmGraphBothStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("records", "kept", "duplicates", "contained", "hits", "edges", "reducible",
                                                 "lookups", "launches", "scratch_bytes", "edge_bytes", "selfrc", "seeds",
                                                 "seed_rows", "tail_hits")] +
                [("edges_kind", ctypes.c_uint64 * 4)] +
                [(n, ctypes.c_float) for n in ("ms_walk", "ms_build", "ms_reduce", "ms_wall", "ms_tail", "ms_merge")])

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["edges_kind"] = list(self.edges_kind)
        return d


class DebwtFmCleanOpts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("max_tip", "max_bubble", "max_rounds", "flags")]


class DebwtFmCleanStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("nodes", "edges", "rounds", "tips", "tip_nodes", "bubbles", "bubble_nodes",
                                                 "steps", "launches")] +
                [(n, ctypes.c_float) for n in ("ms_clean", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmPileAln(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint64), ("tbeg", ctypes.c_uint64), ("qbeg", ctypes.c_uint32), ("strand", ctypes.c_uint32)]


class DebwtFmPileOpts(ctypes.Structure):
    _fields_ = [("min_depth", ctypes.c_uint32), ("min_permille", ctypes.c_uint32)]


class DebwtFmVariant(ctypes.Structure):
    _fields_ = [("t", ctypes.c_uint64), ("depth", ctypes.c_uint32), ("count", ctypes.c_uint32), ("ins", ctypes.c_uint32),
                ("ref", ctypes.c_uint8), ("call", ctypes.c_uint8)]


class DebwtFmInsEvent(ctypes.Structure):
    _fields_ = [("t", ctypes.c_uint64), ("aln", ctypes.c_uint64), ("qpos", ctypes.c_uint32), ("len", ctypes.c_uint32)]


class DebwtFmPileStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("alignments", "ops", "m_columns", "d_bases", "i_ops", "ev_base", "ev_other",
                                                 "ev_del", "ev_ins", "launches", "group", "table_bytes", "call_positions",
                                                 "call_variants")] +
                [(n, ctypes.c_float) for n in ("ms_plan", "ms_kernel", "ms_wall", "ms_call", "ms_call_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmJob(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint64), ("diag", ctypes.c_int64), ("record", ctypes.c_uint32), ("strand", ctypes.c_uint32)]


class DebwtFmScoring(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("match", "mismatch", "gap_open", "gap_extend")]


class DebwtFmAln(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("qbeg", ctypes.c_uint32), ("qend", ctypes.c_uint32), ("edits", ctypes.c_uint32),
                ("tbeg", ctypes.c_uint64), ("tend", ctypes.c_uint64)]


class DebwtFmSeed(ctypes.Structure):
    _fields_ = [("diag", ctypes.c_int64), ("record", ctypes.c_uint32), ("strand", ctypes.c_uint32), ("qbeg", ctypes.c_uint32),
                ("qend", ctypes.c_uint32)]


class DebwtFmCand(ctypes.Structure):
    _fields_ = [("diag", ctypes.c_int64), ("first_diag", ctypes.c_int64), ("record", ctypes.c_uint32),
                ("strand", ctypes.c_uint32), ("weight", ctypes.c_uint32), ("seeds", ctypes.c_uint32)]


class DebwtFmMapOpts(ctypes.Structure):
    _fields_ = [("min_len", ctypes.c_uint32), ("band", ctypes.c_uint32), ("max_occ", ctypes.c_uint32),
                ("max_cand", ctypes.c_uint32), ("min_score", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("scoring", DebwtFmScoring)]


class DebwtFmHit(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("record", ctypes.c_uint32),
                ("offset", ctypes.c_uint64), ("qbeg", ctypes.c_uint32), ("qend", ctypes.c_uint32), ("tbeg", ctypes.c_uint64),
                ("tend", ctypes.c_uint64), ("score", ctypes.c_int32), ("sub", ctypes.c_int32), ("mapq", ctypes.c_uint32),
                ("edits", ctypes.c_uint32), ("diag", ctypes.c_int64)]


class DebwtFmAnchor(ctypes.Structure):
    _fields_ = [("qbeg", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("diag", ctypes.c_int64)]


class DebwtFmChain(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("record", ctypes.c_uint32), ("strand", ctypes.c_uint32),
                ("n_anchors", ctypes.c_uint32), ("first_anchor", ctypes.c_uint64)]


class DebwtFmChainJob(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint64), ("record", ctypes.c_uint32), ("strand", ctypes.c_uint32),
                ("first_anchor", ctypes.c_uint64), ("n_anchors", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DebwtFmChainOpts(ctypes.Structure):
    _fields_ = [("map", DebwtFmMapOpts), ("max_gap", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DebwtFmWindowJob(ctypes.Structure):
    _fields_ = [("pattern", ctypes.c_uint64), ("record", ctypes.c_uint32), ("strand", ctypes.c_uint32),
                ("wbeg", ctypes.c_uint64), ("wend", ctypes.c_uint64)]


class DebwtFmPcand(ctypes.Structure):
    _fields_ = [("score", ctypes.c_int32), ("record", ctypes.c_uint32), ("strand", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("tbeg", ctypes.c_uint64), ("tend", ctypes.c_uint64)]


class DebwtFmPairChoice(ctypes.Structure):
    _fields_ = [("i1", ctypes.c_int32), ("i2", ctypes.c_int32), ("proper", ctypes.c_uint32), ("mapq1", ctypes.c_uint32),
                ("mapq2", ctypes.c_uint32), ("sub1", ctypes.c_int32), ("sub2", ctypes.c_int32), ("pair_score", ctypes.c_int32),
                ("pair_sub", ctypes.c_int32), ("tlen", ctypes.c_int64)]


class DebwtFmPairOpts(ctypes.Structure):
    _fields_ = [("map", DebwtFmMapOpts), ("ins_lo", ctypes.c_uint32), ("ins_hi", ctypes.c_uint32),
                ("max_rescue", ctypes.c_uint32), ("unpaired_penalty", ctypes.c_int32)]


class DebwtFmPairInfo(ctypes.Structure):
    _fields_ = [("tlen", ctypes.c_int64), ("pair_score", ctypes.c_int32), ("pair_sub", ctypes.c_int32),
                ("reserved", ctypes.c_uint32)]


class DebwtFmPairStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("pairs", "proper", "rescue_jobs", "rescued", "ins_lo", "ins_hi",
                                                "estimate_pairs")] +
                [(n, ctypes.c_float) for n in ("ms_candidates", "ms_rescue", "ms_select", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmExtendStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("jobs", "batches", "launches", "cells", "wave_steps", "scratch_bytes")] +
                [(n, ctypes.c_float) for n in ("ms_kernel", "ms_trace", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtFmMapStats(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_uint64) for n in ("reads", "mapped", "mems", "seeds", "candidates", "jobs", "batches")] +
                [(n, ctypes.c_float) for n in ("ms_mems", "ms_locate", "ms_candidates", "ms_extend", "ms_wall")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DebwtMultiStats(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("nrec", ctypes.c_uint64), ("ngpus", ctypes.c_uint32), ("rounds", ctypes.c_uint32),
                ("key_bytes_in", ctypes.c_uint64), ("blue_bytes_in", ctypes.c_uint64), ("ms_build", ctypes.c_float),
                ("key_mode", ctypes.c_uint32), ("exchange_backend", ctypes.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# every symbol include/debwt_hip.h declares
SYMBOLS = [
    "debwt_create", "debwt_destroy", "debwt_strerror", "debwt_last_error", "debwt_load_text",
    "debwt_load_ascii", "debwt_kmer_sort_rle", "debwt_classify", "debwt_sp_generate", "debwt_blue_sort",
    "debwt_bwt_assemble", "debwt_build", "debwt_fetch_bwt", "debwt_bwt_device_ptr", "debwt_get_stats",
    "debwt_fetch_array", "debwt_kmer_count_sorted", "debwt_radix_sort_u64", "debwt_radix_sort_u64_range", "debwt_radix_pair_passes", "debwt_radix_bucket_passes", "debwt_radix_low_finishes", "debwt_verify_inverse",
    "debwt_shard_begin", "debwt_shard_histogram", "debwt_shard_set_range", "debwt_shard_classify_local",
    "debwt_shard_facts_export", "debwt_shard_classify_global", "debwt_shard_info", "debwt_shard_fetch",
    "debwt_shard_partition_keys", "debwt_shard_plan", "debwt_shard_ranges", "debwt_shard_sort_begin",
    "debwt_shard_sort_range", "debwt_shard_sort_end", "debwt_concat_rows", "debwt_shard_export", "debwt_census_words", "debwt_shard_sp_flags", "debwt_shard_sp_emit",
    "debwt_shard_sp_import", "debwt_shard_blue_route", "debwt_shard_blue_place", "debwt_set_range_cap", "debwt_pack_fasta", "debwt_free_packed", "debwt_load_fasta", "debwt_pack_fasta_opts", "debwt_load_fasta_opts", "debwt_fasta_text_bound", "debwt_host_release_hold", "debwt_special_digest", "debwt_bwt_census", "debwt_fetch_rows", "debwt_verify_device", "debwt_multi_create", "debwt_multi_destroy", "debwt_multi_last_error",
    "debwt_multi_load_text", "debwt_multi_load_fasta", "debwt_multi_build", "debwt_multi_fetch_bwt", "debwt_multi_get_stats",
    "debwt_multi_verify", "debwt_multi_shard", "debwt_pinned_alloc", "debwt_pinned_free", "debwt_shard_key_mode",
    "debwt_multi_set_key_mode", "debwt_special_compare", "debwt_build_to_host", "debwt_multi_set_exchange", "debwt_reserve",
    "debwt_multi_set_serial", "debwt_multi_get_shard_report", "debwt_multi_step_name", "debwt_get_config",
    "debwt_dump_reference_files", "debwt_shard_scratch",
    "debwt_fm_create", "debwt_fm_open", "debwt_fm_last_error", "debwt_fm_info_get", "debwt_fm_samples",
    "debwt_fm_record_starts", "debwt_fm_count", "debwt_fm_locate", "debwt_fm_destroy",
    "debwt_fm_search", "debwt_fm_search_stats_get", "debwt_fm_mems", "debwt_fm_mems_stats_get",
    "debwt_fm_attach_text", "debwt_fm_extend", "debwt_fm_extend_stats_get", "debwt_fm_cluster_seeds",
    "debwt_fm_map_defaults", "debwt_fm_map", "debwt_fm_map_stats_get",
    "debwt_fm_chain_seeds", "debwt_fm_extend_chain", "debwt_fm_chain_defaults", "debwt_fm_map_chained",
    "debwt_fm_align_window", "debwt_fm_insert_bounds", "debwt_fm_pair_select", "debwt_fm_pair_defaults",
    "debwt_fm_map_pairs", "debwt_fm_pair_stats_get",
    "debwt_fm_overlaps", "debwt_fm_overlaps_stats_get", "debwt_fm_overlap_longest",
    "debwt_fm_overlaps_mm", "debwt_fm_overlaps_mm_stats_get",
    "debwt_fm_extract", "debwt_fm_extract_stats_get", "debwt_fm_restore_text", "debwt_fm_text_fetch",
    "debwt_fm_kmer_counts", "debwt_fm_kmer_stats_get", "debwt_fm_weak_trials", "debwt_fm_correct_defaults",
    "debwt_fm_correct", "debwt_fm_correct_stats_get",
    "debwt_fm_spectrum", "debwt_fm_kmer_list", "debwt_fm_spectrum_threshold", "debwt_fm_spectrum_stats_get",
    "debwt_fm_esa_build", "debwt_fm_esa_fetch", "debwt_fm_esa_summary_get", "debwt_fm_esa_profile", "debwt_fm_esa_release",
    "debwt_fm_esa_stats_get", "debwt_fm_repeats", "debwt_fm_repeat_stats_get",
    "debwt_fm_records_build", "debwt_fm_records_fetch", "debwt_fm_record_counts", "debwt_fm_repeats_records",
    "debwt_fm_records_stats_get", "debwt_fm_cdbg", "debwt_fm_cdbg_stats_get", "debwt_fm_cdbg_both",
    "debwt_fm_cdbg_both_stats_get",
    "debwt_fm_string_graph", "debwt_fm_edges_reduce", "debwt_fm_unitigs", "debwt_fm_graph_stats_get",
    "debwt_fm_string_graph_both", "debwt_fm_unitigs_both", "debwt_fm_graph_both_stats_get",
    "debwt_fm_clean_defaults", "debwt_fm_graph_clean", "debwt_fm_edges_compact", "debwt_fm_clean_stats_get",
    "debwt_fm_pileup", "debwt_fm_pile_fetch", "debwt_fm_pile_release", "debwt_fm_pile_defaults", "debwt_fm_pile_call",
    "debwt_fm_pile_insertions", "debwt_fm_ins_vote", "debwt_fm_consensus", "debwt_fm_pile_stats_get",
]


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    args = ["make", "-C", src_dir]
    if force:
        subprocess.check_call(args + ["clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C debwt_amd/csrc` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    try:
        import torch  # noqa: F401  (its bundled HIP runtime must be the one in the process, see __graft_entry__.build)
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
    L.debwt_create.restype = ctypes.c_int
    L.debwt_create.argtypes = [ctypes.POINTER(DebwtConfig), ctypes.POINTER(vp)]
    L.debwt_destroy.restype = None
    L.debwt_destroy.argtypes = [vp]
    L.debwt_strerror.restype = ctypes.c_char_p
    L.debwt_strerror.argtypes = [ctypes.c_int]
    L.debwt_last_error.restype = ctypes.c_char_p
    L.debwt_last_error.argtypes = [vp]
    L.debwt_load_text.restype = ctypes.c_int
    L.debwt_load_text.argtypes = [vp, u64p, ctypes.c_uint64, u64p, ctypes.c_uint64]
    L.debwt_load_ascii.restype = ctypes.c_int
    L.debwt_load_ascii.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64]
    for name in ("debwt_kmer_sort_rle", "debwt_classify", "debwt_sp_generate", "debwt_blue_sort",
                 "debwt_bwt_assemble", "debwt_build"):
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [vp]
    L.debwt_fetch_bwt.restype = ctypes.c_int
    L.debwt_fetch_bwt.argtypes = [vp, u64p, u64p, u64p]
    L.debwt_reserve.restype = ctypes.c_int
    L.debwt_reserve.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_double, ctypes.c_uint]
    L.debwt_build_to_host.restype = ctypes.c_int
    L.debwt_build_to_host.argtypes = [vp, u64p, u64p, u64p]
    L.debwt_bwt_device_ptr.restype = ctypes.c_int
    L.debwt_bwt_device_ptr.argtypes = [vp, ctypes.POINTER(vp)]
    L.debwt_get_stats.restype = ctypes.c_int
    L.debwt_get_stats.argtypes = [vp, ctypes.POINTER(DebwtStats)]
    L.debwt_fetch_array.restype = ctypes.c_int
    L.debwt_fetch_array.argtypes = [vp, ctypes.c_int, vp, ctypes.c_uint64, u64p]
    L.debwt_kmer_count_sorted.restype = ctypes.c_int
    L.debwt_kmer_count_sorted.argtypes = [vp, u64p, u64p, ctypes.c_uint64, u64p]
    L.debwt_radix_sort_u64.restype = ctypes.c_int
    L.debwt_radix_sort_u64.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.debwt_radix_pair_passes.restype = ctypes.c_uint64
    L.debwt_radix_pair_passes.argtypes = []
    L.debwt_radix_bucket_passes.restype = ctypes.c_uint64
    L.debwt_radix_bucket_passes.argtypes = []
    L.debwt_radix_low_finishes.restype = ctypes.c_uint64
    L.debwt_radix_low_finishes.argtypes = []
    L.debwt_radix_sort_u64_range.restype = ctypes.c_int
    L.debwt_radix_sort_u64_range.argtypes = [vp, vp, vp, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.POINTER(ctypes.c_float)]
    L.debwt_verify_inverse.restype = ctypes.c_int
    L.debwt_verify_inverse.argtypes = [u64p, ctypes.c_uint64, u64p, ctypes.c_uint64, ctypes.c_uint64,
                                       ctypes.POINTER(ctypes.c_uint8)]
    L.debwt_shard_begin.restype = ctypes.c_int
    L.debwt_shard_begin.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.debwt_shard_histogram.restype = ctypes.c_int
    L.debwt_shard_histogram.argtypes = [vp, u64p]
    L.debwt_shard_set_range.restype = ctypes.c_int
    L.debwt_shard_set_range.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]
    L.debwt_shard_classify_local.restype = ctypes.c_int
    L.debwt_shard_classify_local.argtypes = [vp, u64p, u64p, u64p]
    L.debwt_shard_facts_export.restype = ctypes.c_int
    L.debwt_shard_facts_export.argtypes = [vp, vp, ctypes.c_uint64]
    L.debwt_shard_classify_global.restype = ctypes.c_int
    L.debwt_shard_classify_global.argtypes = [vp, vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    L.debwt_shard_partition_keys.restype = ctypes.c_int
    L.debwt_shard_partition_keys.argtypes = [vp, u8p, vp, ctypes.c_uint64, u64p]
    L.debwt_shard_plan.restype = ctypes.c_int
    L.debwt_shard_plan.argtypes = [vp, u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int,
                                   ctypes.c_uint64, u32p]
    L.debwt_shard_key_mode.restype = ctypes.c_int
    L.debwt_shard_key_mode.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_double)]
    L.debwt_multi_set_key_mode.restype = ctypes.c_int
    L.debwt_multi_set_key_mode.argtypes = [vp, ctypes.c_int]
    L.debwt_multi_set_exchange.restype = ctypes.c_int
    L.debwt_multi_set_exchange.argtypes = [vp, ctypes.c_int]
    L.debwt_shard_ranges.restype = ctypes.c_int
    L.debwt_shard_ranges.argtypes = [vp, u32p, u64p, ctypes.c_uint32]
    L.debwt_shard_sort_begin.restype = ctypes.c_int
    L.debwt_shard_sort_begin.argtypes = [vp]
    L.debwt_shard_sort_range.restype = ctypes.c_int
    L.debwt_shard_sort_range.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint64]
    L.debwt_shard_sort_end.restype = ctypes.c_int
    L.debwt_shard_sort_end.argtypes = [vp]
    L.debwt_shard_export.restype = ctypes.c_int
    L.debwt_shard_export.argtypes = [vp, vp, ctypes.c_uint64]
    L.debwt_census_words.restype = ctypes.c_int
    L.debwt_census_words.argtypes = [vp, vp, ctypes.c_uint64, u64p]
    L.debwt_concat_rows.restype = ctypes.c_int
    L.debwt_concat_rows.argtypes = [vp, vp, ctypes.c_uint32, u64p, u64p, u64p, ctypes.c_uint64, vp]
    L.debwt_shard_sp_flags.restype = ctypes.c_int
    L.debwt_shard_sp_flags.argtypes = [vp, u64p, u64p]
    L.debwt_shard_sp_emit.restype = ctypes.c_int
    L.debwt_shard_sp_emit.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint64]
    L.debwt_shard_sp_import.restype = ctypes.c_int
    L.debwt_shard_sp_import.argtypes = [vp, vp, ctypes.c_uint64]
    L.debwt_shard_blue_route.restype = ctypes.c_int
    L.debwt_shard_blue_route.argtypes = [vp, u32p, vp, ctypes.c_uint64, u64p]
    L.debwt_shard_blue_place.restype = ctypes.c_int
    L.debwt_shard_blue_place.argtypes = [vp, vp, ctypes.c_uint64]
    L.debwt_shard_info.restype = ctypes.c_int
    L.debwt_shard_info.argtypes = [vp, u64p, u64p, u64p]
    L.debwt_shard_fetch.restype = ctypes.c_int
    L.debwt_shard_fetch.argtypes = [vp, u64p, u64p, u64p]
    L.debwt_pack_fasta.restype = ctypes.c_int
    L.debwt_pack_fasta.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(DebwtPackedText), ctypes.c_char_p,
                                   ctypes.c_size_t]
    L.debwt_free_packed.restype = None
    L.debwt_free_packed.argtypes = [ctypes.POINTER(DebwtPackedText)]
    L.debwt_load_fasta.restype = ctypes.c_int
    L.debwt_load_fasta.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
    L.debwt_host_release_hold.restype = None
    L.debwt_host_release_hold.argtypes = [ctypes.c_int]
    L.debwt_fasta_text_bound.restype = ctypes.c_uint64
    L.debwt_fasta_text_bound.argtypes = [ctypes.c_char_p]
    L.debwt_pack_fasta_opts.restype = ctypes.c_int
    L.debwt_pack_fasta_opts.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint64,
                                        ctypes.POINTER(DebwtPackedText), ctypes.c_char_p, ctypes.c_size_t]
    L.debwt_load_fasta_opts.restype = ctypes.c_int
    L.debwt_load_fasta_opts.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint64]
    L.debwt_special_compare.restype = ctypes.c_int
    L.debwt_special_compare.argtypes = [vp, u64p]
    L.debwt_special_digest.restype = ctypes.c_int
    L.debwt_special_digest.argtypes = [u64p, ctypes.c_uint64, u64p, ctypes.c_uint64, ctypes.c_int, u64p]
    L.debwt_multi_create.restype = ctypes.c_int
    L.debwt_multi_create.argtypes = [ctypes.POINTER(DebwtConfig), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(vp)]
    L.debwt_multi_destroy.restype = None
    L.debwt_multi_destroy.argtypes = [vp]
    L.debwt_multi_last_error.restype = ctypes.c_char_p
    L.debwt_multi_last_error.argtypes = [vp]
    L.debwt_multi_load_text.restype = ctypes.c_int
    L.debwt_multi_load_text.argtypes = [vp, u64p, ctypes.c_uint64, u64p, ctypes.c_uint64]
    L.debwt_multi_load_fasta.restype = ctypes.c_int
    L.debwt_multi_load_fasta.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint64]
    L.debwt_multi_build.restype = ctypes.c_int
    L.debwt_multi_build.argtypes = [vp]
    L.debwt_multi_fetch_bwt.restype = ctypes.c_int
    L.debwt_multi_fetch_bwt.argtypes = [vp, u64p, u64p, u64p]
    L.debwt_multi_get_stats.restype = ctypes.c_int
    L.debwt_multi_get_stats.argtypes = [vp, ctypes.POINTER(DebwtMultiStats), ctypes.POINTER(DebwtStats)]
    L.debwt_multi_shard.restype = vp
    L.debwt_multi_shard.argtypes = [vp, ctypes.c_int]
    L.debwt_multi_set_serial.restype = ctypes.c_int
    L.debwt_multi_set_serial.argtypes = [vp, ctypes.c_int]
    L.debwt_multi_get_shard_report.restype = ctypes.c_int
    L.debwt_multi_get_shard_report.argtypes = [vp, ctypes.c_int, ctypes.POINTER(DebwtShardReport)]
    L.debwt_multi_step_name.restype = ctypes.c_char_p
    L.debwt_multi_step_name.argtypes = [ctypes.c_int]
    L.debwt_multi_verify.restype = ctypes.c_int
    L.debwt_multi_verify.argtypes = [vp, ctypes.POINTER(DebwtVerifyReport)]
    L.debwt_verify_device.restype = ctypes.c_int
    L.debwt_verify_device.argtypes = [vp, vp, u64p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(DebwtVerifyReport)]
    L.debwt_fetch_rows.restype = ctypes.c_int
    L.debwt_fetch_rows.argtypes = [vp, u64p, u64p]
    L.debwt_bwt_census.restype = ctypes.c_int
    L.debwt_bwt_census.argtypes = [vp, u64p]
    L.debwt_set_range_cap.restype = ctypes.c_int
    L.debwt_set_range_cap.argtypes = [vp, ctypes.c_uint64]
    L.debwt_shard_scratch.restype = ctypes.c_int
    L.debwt_shard_scratch.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp), u64p]
    L.debwt_get_config.restype = ctypes.c_int
    L.debwt_get_config.argtypes = [vp, ctypes.POINTER(DebwtConfig)]
    L.debwt_dump_reference_files.restype = ctypes.c_int
    L.debwt_dump_reference_files.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
    L.debwt_fm_create.restype = ctypes.c_int
    L.debwt_fm_create.argtypes = [vp, u64p, u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(vp)]
    L.debwt_fm_open.restype = ctypes.c_int
    L.debwt_fm_open.argtypes = [ctypes.c_int, u64p, ctypes.c_uint64, u64p, ctypes.c_uint64, ctypes.c_uint64, u64p,
                                ctypes.c_uint32, ctypes.POINTER(vp)]
    L.debwt_fm_last_error.restype = ctypes.c_char_p
    L.debwt_fm_last_error.argtypes = [vp]
    L.debwt_fm_info_get.restype = ctypes.c_int
    L.debwt_fm_info_get.argtypes = [vp, ctypes.POINTER(DebwtFmInfo)]
    L.debwt_fm_samples.restype = ctypes.c_int
    L.debwt_fm_samples.argtypes = [vp, u64p, ctypes.c_uint64]
    L.debwt_fm_record_starts.restype = ctypes.c_int
    L.debwt_fm_record_starts.argtypes = [vp, u64p, ctypes.c_uint64]
    L.debwt_fm_count.restype = ctypes.c_int
    L.debwt_fm_count.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, u64p]
    L.debwt_fm_locate.restype = ctypes.c_int
    L.debwt_fm_locate.argtypes = [vp, u64p, ctypes.c_uint64, ctypes.c_uint64, u64p, u64p, ctypes.c_uint64]
    L.debwt_fm_search.restype = ctypes.c_int
    L.debwt_fm_search.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p, u64p,
                                  ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
    L.debwt_fm_search_stats_get.restype = ctypes.c_int
    L.debwt_fm_search_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmSearchStats)]
    L.debwt_fm_mems.restype = ctypes.c_int
    L.debwt_fm_mems.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p,
                                ctypes.POINTER(ctypes.c_uint32), u64p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint64]
    L.debwt_fm_mems_stats_get.restype = ctypes.c_int
    L.debwt_fm_mems_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmMemsStats)]
    L.debwt_fm_overlaps.restype = ctypes.c_int
    L.debwt_fm_overlaps.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p,
                                    ctypes.POINTER(DebwtFmOverlap), ctypes.c_uint64]
    L.debwt_fm_overlaps_stats_get.restype = ctypes.c_int
    L.debwt_fm_overlaps_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmOverlapsStats)]
    L.debwt_fm_overlaps_mm.restype = ctypes.c_int
    L.debwt_fm_overlaps_mm.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.c_uint32, u64p, ctypes.POINTER(DebwtFmOverlap), ctypes.c_uint64]
    L.debwt_fm_overlaps_mm_stats_get.restype = ctypes.c_int
    L.debwt_fm_overlaps_mm_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmOverlapsMmStats)]
    L.debwt_fm_overlap_longest.restype = ctypes.c_int
    L.debwt_fm_overlap_longest.argtypes = [ctypes.POINTER(DebwtFmOverlap), u64p, ctypes.c_uint64, u64p]
    L.debwt_fm_attach_text.restype = ctypes.c_int
    L.debwt_fm_attach_text.argtypes = [vp, vp, u64p, u64p]
    L.debwt_fm_extend.restype = ctypes.c_int
    L.debwt_fm_extend.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.POINTER(DebwtFmJob), ctypes.c_uint64,
                                  ctypes.POINTER(DebwtFmScoring), ctypes.c_uint32, ctypes.POINTER(DebwtFmAln), u64p,
                                  ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
    L.debwt_fm_extend_stats_get.restype = ctypes.c_int
    L.debwt_fm_extend_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmExtendStats)]
    L.debwt_fm_cluster_seeds.restype = ctypes.c_int
    L.debwt_fm_cluster_seeds.argtypes = [ctypes.POINTER(DebwtFmSeed), ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.POINTER(DebwtFmCand)]
    L.debwt_fm_map_defaults.restype = None
    L.debwt_fm_map_defaults.argtypes = [ctypes.POINTER(DebwtFmMapOpts)]
    L.debwt_fm_map.restype = ctypes.c_int
    L.debwt_fm_map.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.POINTER(DebwtFmMapOpts),
                               ctypes.POINTER(DebwtFmHit), u64p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
    L.debwt_fm_map_stats_get.restype = ctypes.c_int
    L.debwt_fm_map_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmMapStats)]
    L.debwt_fm_chain_seeds.restype = ctypes.c_int
    L.debwt_fm_chain_seeds.argtypes = [ctypes.POINTER(DebwtFmSeed), ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.POINTER(DebwtFmChain), ctypes.POINTER(DebwtFmAnchor),
                                       ctypes.c_uint64, u64p]
    L.debwt_fm_extend_chain.restype = ctypes.c_int
    L.debwt_fm_extend_chain.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.POINTER(DebwtFmChainJob),
                                        ctypes.c_uint64, ctypes.POINTER(DebwtFmAnchor), ctypes.c_uint64,
                                        ctypes.POINTER(DebwtFmScoring), ctypes.c_uint32, ctypes.POINTER(DebwtFmAln), u64p,
                                        ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
    L.debwt_fm_chain_defaults.restype = None
    L.debwt_fm_chain_defaults.argtypes = [ctypes.POINTER(DebwtFmChainOpts)]
    L.debwt_fm_map_chained.restype = ctypes.c_int
    L.debwt_fm_map_chained.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.POINTER(DebwtFmChainOpts),
                                       ctypes.POINTER(DebwtFmHit), u64p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64,
                                       u64p, ctypes.POINTER(DebwtFmAnchor), ctypes.c_uint64]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.debwt_fm_align_window.restype = ctypes.c_int
    L.debwt_fm_align_window.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.POINTER(DebwtFmWindowJob),
                                        ctypes.c_uint64, ctypes.POINTER(DebwtFmScoring), ctypes.POINTER(DebwtFmAln), u64p,
                                        u32p, ctypes.c_uint64]
    L.debwt_fm_insert_bounds.restype = ctypes.c_int
    L.debwt_fm_insert_bounds.argtypes = [u64p, ctypes.c_uint64, u32p, u32p]
    L.debwt_fm_pair_select.restype = ctypes.c_int
    L.debwt_fm_pair_select.argtypes = [ctypes.POINTER(DebwtFmPcand), ctypes.c_uint32, ctypes.POINTER(DebwtFmPcand),
                                       ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.POINTER(DebwtFmPairChoice)]
    L.debwt_fm_pair_defaults.restype = None
    L.debwt_fm_pair_defaults.argtypes = [ctypes.POINTER(DebwtFmPairOpts)]
    L.debwt_fm_map_pairs.restype = ctypes.c_int
    L.debwt_fm_map_pairs.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.POINTER(DebwtFmPairOpts),
                                     ctypes.POINTER(DebwtFmHit), ctypes.POINTER(DebwtFmPairInfo), u64p, u32p, ctypes.c_uint64]
    L.debwt_fm_pair_stats_get.restype = ctypes.c_int
    L.debwt_fm_pair_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmPairStats)]
    L.debwt_fm_extract.restype = ctypes.c_int
    L.debwt_fm_extract.argtypes = [vp, ctypes.POINTER(DebwtFmExtractJob), ctypes.c_uint64, u64p, ctypes.c_char_p, ctypes.c_uint64]
    L.debwt_fm_extract_stats_get.restype = ctypes.c_int
    L.debwt_fm_extract_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmExtractStats)]
    L.debwt_fm_restore_text.restype = ctypes.c_int
    L.debwt_fm_restore_text.argtypes = [vp]
    L.debwt_fm_text_fetch.restype = ctypes.c_int
    L.debwt_fm_text_fetch.argtypes = [vp, u64p, ctypes.c_uint64, u64p]
    L.debwt_fm_kmer_counts.restype = ctypes.c_int
    L.debwt_fm_kmer_counts.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p, u32p,
                                       ctypes.c_uint64]
    L.debwt_fm_kmer_stats_get.restype = ctypes.c_int
    L.debwt_fm_kmer_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmKmerStats)]
    L.debwt_fm_weak_trials.restype = ctypes.c_int
    L.debwt_fm_weak_trials.argtypes = [u32p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(DebwtFmTrial),
                                       ctypes.c_uint64]
    L.debwt_fm_correct_defaults.restype = None
    L.debwt_fm_correct_defaults.argtypes = [ctypes.POINTER(DebwtFmCorrectOpts)]
    L.debwt_fm_correct.restype = ctypes.c_int
    L.debwt_fm_correct.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, ctypes.POINTER(DebwtFmCorrectOpts), vp,
                                   ctypes.POINTER(DebwtFmCorrectInfo)]
    L.debwt_fm_correct_stats_get.restype = ctypes.c_int
    L.debwt_fm_correct_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmCorrectStats)]
    L.debwt_fm_spectrum.restype = ctypes.c_int
    L.debwt_fm_spectrum.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p,
                                    ctypes.POINTER(DebwtFmSpectrumTotals)]
    L.debwt_fm_kmer_list.restype = ctypes.c_int
    L.debwt_fm_kmer_list.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u64p, u32p,
                                     ctypes.c_uint64, u64p]
    L.debwt_fm_spectrum_threshold.restype = ctypes.c_int
    L.debwt_fm_spectrum_threshold.argtypes = [u64p, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(DebwtFmSpectrumSummary)]
    L.debwt_fm_spectrum_stats_get.restype = ctypes.c_int
    L.debwt_fm_spectrum_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmSpectrumStats)]
    L.debwt_fm_esa_build.restype = ctypes.c_int
    L.debwt_fm_esa_build.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32]
    L.debwt_fm_esa_fetch.restype = ctypes.c_int
    L.debwt_fm_esa_fetch.argtypes = [vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    L.debwt_fm_esa_summary_get.restype = ctypes.c_int
    L.debwt_fm_esa_summary_get.argtypes = [vp, ctypes.POINTER(DebwtFmEsaSummary)]
    L.debwt_fm_esa_profile.restype = ctypes.c_int
    L.debwt_fm_esa_profile.argtypes = [vp, ctypes.c_uint32, u64p]
    L.debwt_fm_esa_release.restype = ctypes.c_int
    L.debwt_fm_esa_release.argtypes = [vp]
    L.debwt_fm_esa_stats_get.restype = ctypes.c_int
    L.debwt_fm_esa_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmEsaStats)]
    L.debwt_fm_repeats.restype = ctypes.c_int
    L.debwt_fm_repeats.argtypes = [vp, ctypes.POINTER(DebwtFmRepeatOpts), ctypes.c_void_p, ctypes.c_uint64, u64p]
    L.debwt_fm_repeat_stats_get.restype = ctypes.c_int
    L.debwt_fm_repeat_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmRepeatStats)]
    L.debwt_fm_records_build.restype = ctypes.c_int
    L.debwt_fm_records_build.argtypes = [vp]
    L.debwt_fm_records_fetch.restype = ctypes.c_int
    L.debwt_fm_records_fetch.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, u64p]
    L.debwt_fm_record_counts.restype = ctypes.c_int
    L.debwt_fm_record_counts.argtypes = [vp, u64p, ctypes.c_uint64, u64p]
    L.debwt_fm_repeats_records.restype = ctypes.c_int
    L.debwt_fm_repeats_records.argtypes = [vp, ctypes.POINTER(DebwtFmRepeatOpts), ctypes.POINTER(DebwtFmRecordFilter),
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, u64p]
    L.debwt_fm_records_stats_get.restype = ctypes.c_int
    L.debwt_fm_records_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmRecordsStats)]
    L.debwt_fm_cdbg.restype = ctypes.c_int
    L.debwt_fm_cdbg.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(DebwtFmCdbgSizes)]
    L.debwt_fm_cdbg_stats_get.restype = ctypes.c_int
    L.debwt_fm_cdbg_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmCdbgStats)]
    L.debwt_fm_cdbg_both.restype = ctypes.c_int
    L.debwt_fm_cdbg_both.argtypes = L.debwt_fm_cdbg.argtypes
    L.debwt_fm_cdbg_both_stats_get.restype = ctypes.c_int
    L.debwt_fm_cdbg_both_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmCdbgBothStats)]
    u8p, edgep = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(DebwtFmEdge)
    L.debwt_fm_string_graph.restype = ctypes.c_int
    L.debwt_fm_string_graph.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u8p, u64p, edgep, ctypes.c_uint64]
    L.debwt_fm_edges_reduce.restype = ctypes.c_int
    L.debwt_fm_edges_reduce.argtypes = [vp, u64p, ctypes.c_uint64, u64p, edgep, u8p]
    L.debwt_fm_unitigs.restype = ctypes.c_int
    L.debwt_fm_unitigs.argtypes = [u8p, u64p, edgep, ctypes.c_uint64, u64p, u32p, u8p, u64p]
    L.debwt_fm_graph_stats_get.restype = ctypes.c_int
    L.debwt_fm_graph_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmGraphStats)]
    L.debwt_fm_string_graph_both.restype = ctypes.c_int
    L.debwt_fm_string_graph_both.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u8p, u64p, edgep, ctypes.c_uint64]
    L.debwt_fm_unitigs_both.restype = ctypes.c_int
    L.debwt_fm_unitigs_both.argtypes = [u8p, u64p, edgep, ctypes.c_uint64, u64p, u32p, u8p, u64p]
    L.debwt_fm_graph_both_stats_get.restype = ctypes.c_int
    L.debwt_fm_graph_both_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmGraphBothStats)]
    L.debwt_fm_clean_defaults.restype = None
    L.debwt_fm_clean_defaults.argtypes = [ctypes.POINTER(DebwtFmCleanOpts)]
    L.debwt_fm_graph_clean.restype = ctypes.c_int
    L.debwt_fm_graph_clean.argtypes = [vp, u8p, u64p, edgep, ctypes.c_uint64, ctypes.POINTER(DebwtFmCleanOpts), u8p, u8p]
    L.debwt_fm_edges_compact.restype = ctypes.c_int
    L.debwt_fm_edges_compact.argtypes = [u64p, edgep, u8p, ctypes.c_uint64, u64p, edgep]
    L.debwt_fm_clean_stats_get.restype = ctypes.c_int
    L.debwt_fm_clean_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmCleanStats)]
    alnp, evp = ctypes.POINTER(DebwtFmPileAln), ctypes.POINTER(DebwtFmInsEvent)
    L.debwt_fm_pileup.restype = ctypes.c_int
    L.debwt_fm_pileup.argtypes = [vp, ctypes.c_char_p, u64p, ctypes.c_uint64, alnp, ctypes.c_uint64, u64p, u32p,
                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    L.debwt_fm_pile_fetch.restype = ctypes.c_int
    L.debwt_fm_pile_fetch.argtypes = [vp, u64p, u32p, ctypes.c_uint64]
    L.debwt_fm_pile_release.restype = ctypes.c_int
    L.debwt_fm_pile_release.argtypes = [vp]
    L.debwt_fm_pile_defaults.restype = None
    L.debwt_fm_pile_defaults.argtypes = [ctypes.POINTER(DebwtFmPileOpts)]
    L.debwt_fm_pile_call.restype = ctypes.c_int
    L.debwt_fm_pile_call.argtypes = [vp, ctypes.POINTER(DebwtFmPileOpts), u8p, u8p, ctypes.POINTER(DebwtFmVariant),
                                     ctypes.c_uint64, u64p]
    L.debwt_fm_pile_insertions.restype = ctypes.c_int
    L.debwt_fm_pile_insertions.argtypes = [vp, ctypes.c_uint64, u64p, alnp, ctypes.c_uint64, u64p, u32p, u64p, ctypes.c_uint64,
                                           evp, ctypes.c_uint64, u64p]
    L.debwt_fm_ins_vote.restype = ctypes.c_int
    L.debwt_fm_ins_vote.argtypes = [ctypes.c_char_p, u64p, ctypes.c_uint64, alnp, ctypes.c_uint64, evp, ctypes.c_uint64,
                                    ctypes.c_char_p, ctypes.c_uint64, u64p, u32p]
    L.debwt_fm_consensus.restype = ctypes.c_int
    L.debwt_fm_consensus.argtypes = [u8p, u8p, ctypes.c_uint64, ctypes.c_uint64, u64p, u64p, ctypes.c_char_p, u32p, u32p,
                                     ctypes.c_uint64, ctypes.c_uint32, u64p, ctypes.c_uint64, ctypes.c_uint64, u64p,
                                     ctypes.c_char_p, ctypes.c_uint64]
    L.debwt_fm_pile_stats_get.restype = ctypes.c_int
    L.debwt_fm_pile_stats_get.argtypes = [vp, ctypes.POINTER(DebwtFmPileStats)]
    L.debwt_fm_destroy.restype = None
    L.debwt_fm_destroy.argtypes = [vp]
    _lib = L
    return L
