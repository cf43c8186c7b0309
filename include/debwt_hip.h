/*
 * debwt_hip.h -- C ABI of libdebwt_hip.so, the MI355X (gfx950) implementation of deBWT's
 * de Bruijn branch-encode suffix sort and BWT assembly path.
 *
 * The reference has no plugin/FFI interface: its stages are C functions that pass state through
 * ~30 globals and temp files and exit(1) on error (/root/reference/src/main.h:1-8,
 * src/main.c:79-160).  Each entry point below replaces one of those stage calls; the comment on
 * each names the call it replaces.  Conventions that differ from the reference on purpose:
 *   - an opaque context instead of globals; explicit caller-owned buffers with sizes;
 *   - every function returns int: 0 = ok, negative = DEBWT_E* (never exits, never prints);
 *   - no temp files, no Jellyfish: k-mers are enumerated from the packed text on the GPU;
 *   - functions are not re-entrant on one context; one host thread drives one context/GPU.
 *
 * Data formats are the reference's: text 2 bits/base A0 C1 G2 T3, 32 bases per
 * uint64_t, base j at bit 2*(31-(j&31)) of word j>>5, 'T' stored at every separator and 32 'T'
 * of padding after the end (src/collect#$.c:61-90); BWT output in the same packing with '#'/'$'
 * rows stored as 3 and listed separately (src/insertCase3.c:75-97,115-131).
 */
#ifndef DEBWT_HIP_H
#define DEBWT_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DEBWT_OK 0
#define DEBWT_EINVAL (-1)   /* bad argument (k outside 12..32, n too small, NULL pointer, ...) */
#define DEBWT_ENOMEM (-2)   /* device or host allocation failed */
#define DEBWT_EDEVICE (-3)  /* HIP runtime error (see debwt_last_error) */
#define DEBWT_ESTATE (-4)   /* stage called out of order */
#define DEBWT_ERANGE (-5)   /* input exceeds a capacity of this build (see debwt_last_error) */
#define DEBWT_EINTERNAL (-6)/* consistency check failed */
#define DEBWT_EIO (-7)      /* a file could not be created or written (debwt_dump_reference_files) */

typedef struct debwt_ctx debwt_ctx;

typedef struct {
    int k;          /* edge length, KMER_LENGTH_PlusOne, 12..32 (src/main.c:41-47); node = k-1 */
    int device;     /* HIP device ordinal */
    int sort_algo;  /* 0 = default (3); 1 = all digits by LSD passes in HBM; 3 = top digits in HBM, rest in LDS */
    int reserved;
} debwt_config;

/* counters of one run; the first block mirrors the reference's globals so that runs can be
 * compared stage by stage (src/generateSP.c:28-31, src/collect#$.c:59) */
typedef struct {
    uint64_t n;                 /* BWTLEN */
    uint64_t nrec;              /* countRead */
    uint64_t red_capacity;      /* redCapacity */
    uint64_t blue_capacity;     /* blueCapacity */
    uint64_t blue_bound_num;    /* blueBoundNum */
    uint64_t case3num;          /* case3num */
    uint64_t sp_len;            /* SP symbols (spCodeLen - 32) */
    uint64_t special_branch_num;/* specialBranchNum */
    uint64_t n_main;            /* node instances sorted (n - nrec*(k-1)) */
    uint64_t distinct_keys;     /* distinct (node,pred) keys incl. record-start instances */
    uint64_t blue_large_blocks; /* blocks sorted by the global-memory path */
    uint64_t blue_max_block;
    /* device time of the last run, milliseconds (hipEvents on the context's stream) */
    float ms_extract, ms_sort, ms_classify, ms_sp, ms_blue, ms_assemble, ms_total, ms_host_special;
    /* dominant kernel (one radix scatter pass): launches and total ms in the last run */
    uint32_t radix_pass_launches;
    float radix_pass_ms;
    uint64_t radix_pass_keys;   /* keys moved per launch */
    /* how the special-region tables of the last run were built (collect, src/collect#$.c:118-157,348-602):
     * special_path 0 = one host thread, 1 = host threads, 2 = device; special_threads = host threads used */
    uint32_t special_path, special_threads;
    /* bucket finish of the key sort (all key ranges of the last run): stretches above a wave tile (1024 keys), those of
     * them the classifying kernel left to the 4096-key network, stretches above 4096 keys (all-HBM passes) */
    uint64_t sort_unfit_stretches, sort_unfit_network, sort_over_stretches;
    /* key ranges of the last run whose lowest prefix digit was split bucket by bucket in LDS instead of by an HBM pass */
    uint64_t sort_bucket_passes;
} debwt_stats;

int debwt_create(const debwt_config *cfg, debwt_ctx **out);
void debwt_destroy(debwt_ctx *ctx);
const char *debwt_strerror(int code);
const char *debwt_last_error(const debwt_ctx *ctx);   /* text of the last HIP/internal failure */
int debwt_get_config(const debwt_ctx *ctx, debwt_config *out);   /* the configuration the context was created with */

/* Replaces `collect`'s text hand-over (src/collect#$.c:61-90,100-113: files `reference`,
 * `specialSA`).  packed: ceil((n+32)/32) words in the format above (host memory, must stay valid
 * until the context is destroyed or the next load); sep: the nrec separator positions ascending,
 * sep[nrec-1] == n-1 ('$').  Copies the text to HBM and sizes the workspace. */
int debwt_load_text(debwt_ctx *ctx, const uint64_t *packed, uint64_t n, const uint64_t *sep, uint64_t nrec);

/* Convenience for hosts that hold ASCII: records concatenated without separators, upper or
 * lower case ACGT only (src/main.c:18-23), every record > 32 bases (src/collect#$.c:41-45).
 * Packs on the host, then behaves like debwt_load_text (the packed copy is owned by ctx). */
int debwt_load_ascii(debwt_ctx *ctx, const char *seq, const uint64_t *reclen, uint64_t nrec);

/* FASTA ingest (replaces the reference's single-threaded kseq.h + zlib reader, src/collect#$.c:34-90): the file is
 * mapped (gzip: inflated), parsed and packed by `threads` host threads (the reference's -t) into the text format
 * above.  FASTQ (first byte '@') is read as the reference's reader reads it (src/kseq.h:177-201: sequence lines up to a
 * line that starts with '+', '@' or '>'; after '+' as many quality characters as bases, which are dropped; records
 * without a quality section and '>' records may be mixed in).  Characters other than ACGTacgt and white
 * space, sequence before the first header, a quality string of another length than its sequence and records of 32 bases
 * or fewer (src/collect#$.c:41-45) are errors.  debwt_pack_fasta is host-only (no GPU needed);
 * debwt_load_fasta = debwt_pack_fasta + debwt_load_text with the packed copy owned by ctx. */
typedef struct {
    uint64_t *words;      /* ((n + 63) >> 5) + 2 words */
    uint64_t nwords;
    uint64_t n;           /* BWTLEN */
    uint64_t *sep;        /* nrec separator positions, sep[nrec-1] == n-1 */
    uint64_t nrec;
    double seconds_read, seconds_pack;
} debwt_packed_text;
int debwt_pack_fasta(const char *path, int threads, debwt_packed_text *out, char *errbuf, size_t errlen);
void debwt_free_packed(debwt_packed_text *p);
int debwt_load_fasta(debwt_ctx *ctx, const char *path, int threads);
/* The same with options.  DEBWT_FASTA_IUPAC_RANDOM: N and the other IUPAC ambiguity letters are replaced by one of the
 * bases they stand for -- what the reference leaves to otherTool/transferN.c (:8-32 tables, :57-60 draw with rand()),
 * made deterministic: the draw is a hash of `seed` and the base's text position, independent of the thread count. */
#define DEBWT_FASTA_IUPAC_RANDOM 1u
int debwt_pack_fasta_opts(const char *path, int threads, unsigned flags, uint64_t seed, debwt_packed_text *out,
                          char *errbuf, size_t errlen);
int debwt_load_fasta_opts(debwt_ctx *ctx, const char *path, int threads, unsigned flags, uint64_t seed);
/* An upper bound of the text length (symbols incl. separators) the file can hold, from its size and framing alone -- a plain
 * file: its bytes; block gzip: the members' ISIZE added up; one gzip member below 1 GB: its ISIZE -- or 0 when that cannot be
 * told (several plain members, a large member).  For the n of a debwt_reserve that runs beside the parse; a text that turns out
 * longer only makes the buffers grow at the load.  (The reference knows its text's length only after reading it,
 * src/collect#$.c:52-59.) */
uint64_t debwt_fasta_text_bound(const char *path);
/* The ingest of a gzip file gives up buffers as large as the text (inflated text, pieces); the library releases them on a thread
 * of its own once the text is packed -- returning memory costs this host's kernel 50 ms per GB, and it holds the address space's
 * lock meanwhile.  Between debwt_host_release_hold(1) and (0) nothing is released: a host that copies the packed text to the
 * device right behind the parse (debwt_load_text from pageable memory) brackets both.  Calls nest. */
void debwt_host_release_hold(int on);

/* Device memory for a text of up to n symbols in nrec records, allocated before the text is there: a one-shot host (the
 * reference is one: src/main.c:16-173) calls this on a helper thread while it still reads and packs its input, so that the
 * seconds the driver takes to hand out a few hundred GB (it clears what another process released) pass behind the
 * ingest instead of inside the first build.  branching: expected fraction of positions that are branching nodes, sizes the
 * data-dependent buffers (<= 0: 0.12); everything grows later if the text needs more.  Optional: without it the same
 * buffers are allocated by debwt_load_text and the stages.  Not re-entrant with other calls on the context; DEBWT_ESTATE
 * on a context that already holds a text (its buffers would be re-allocated under it).
 * DEBWT_RESERVE_ONE_SHOT: the context will build once.  When the first buffers arrive at the driver's clearing rate (the
 * memory was another process's a moment ago) the text is cut into more, smaller key ranges than a context that is reused
 * would take -- less workspace to wait for, a few more passes over the text.  That choice STAYS with the context for every
 * later build, exactly like a debwt_set_range_cap (which also undoes it). */
#define DEBWT_RESERVE_ONE_SHOT 1u
/* DEBWT_RESERVE_COMPACT: key ranges of 2^29 instances at most (up to 16 ranges), whatever the first buffers cost: a process
 * that runs right behind another one is handed memory the driver is still clearing, and waits for ALL of the clearing as soon as
 * one of its buffers lies in it -- a third of the workspace mostly comes from memory that is clean.  3.1 Gbp: 28 GiB of device
 * memory instead of 102, 8 % more time per build: cli/deBWT right behind another run 0.9 s instead of 4.3 s.  Texts above 20 Gbp
 * are left to ONE_SHOT's rule (their text-sized buffers alone fill half the device).  cli/deBWT asks for it; like ONE_SHOT the
 * choice stays with the context. */
#define DEBWT_RESERVE_COMPACT 2u
int debwt_reserve(debwt_ctx *ctx, uint64_t n, uint64_t nrec, double branching, unsigned flags);

/* Texts whose node instances (one 8-byte key per base) do not fit HBM at once, or number 2^32 or more, are built
 * in key ranges: prefix ranges of the k-mer space holding at most `max_instances` keys each, sorted and classified
 * one after the other over the resident 2-bit text -- the single-GPU form of SURVEY 8e's bucket sharding (the
 * reference's analogue is its per-thread bucket segments, src/mySort.c:98-110).  Default 2^31; tests lower it to
 * drive the multi-range path on small inputs.  The result does not depend on it. */
int debwt_set_range_cap(debwt_ctx *ctx, uint64_t max_instances);

/* ---- stage entry points, to be called in this order after a load ------------------------------ */
/* Capacities of this build (the reference has none: uint64_t throughout, src/collect#$.h) -- each is a 32-bit index somewhere,
 * each answers DEBWT_ERANGE with the reason in debwt_last_error, none has a slower fall-back:
 *   debwt_kmer_sort_rle / debwt_shard_plan  one 12-mer prefix bin (the unit key ranges are cut at) holds 2^32 - 2^20 node
 *                        instances or more: a key range indexes its keys with 32 bits.  30 Gbp of ten genomes: the fullest
 *                        bin holds 0.1 G; a text of > 4 G copies of one 12-mer (a 4 Gbp homopolymer) would hit it.
 *   debwt_sp_generate    more than 2^31 branching nodes (slot numbers of the node table are 32-bit: 2^32 slots = 64 GB;
 *                        k = 16 on 3.1 Gbp has 0.7 G); a sharded build: a text slice with 2^32 multi-in positions or more
 *                        (debwt_shard_blue_route; ten genomes with an Alu-like family at N = 1: use more shards or the
 *                        one-GPU build, which buckets its 5.6 G entries by key range), or a routed entry whose block id
 *                        and SP index do not fit 61 bits (debwt_shard_sp_emit).
 *   debwt_shard_begin    world > 255 (the owner table holds bytes).
 * DEBWT_ENOMEM is not a capacity: the stages release what the other stages left (debwt_hip.hip, reclaim) before they give up. */

/* Replaces kmercounting.sh + mySort (src/main.c:70,83; src/mySort.c:26-201) and getKmer
 * (src/getKmer.c:12-49): enumerates every node instance of the text as a key
 * (node << 2 | predecessor base) -- the edge list grouped by its (k-1)-suffix, i.e. getKmer's
 * multiIn{A,C,G,T} view -- radix-sorts the keys and run-length encodes them. */
int debwt_kmer_sort_rle(debwt_ctx *ctx);
/* Replaces generateBlocks/mergeKmer (src/INandOut.c:13-89,159-943) plus the special-region
 * tables of collect (src/collect#$.c:118-157,348-602): node flags, red table, block bounds,
 * case-2 characters, rows of the special suffixes. */
int debwt_classify(debwt_ctx *ctx);
/* Replaces generateSP (src/generateSP.c:19-272): SP code and blue entries. */
int debwt_sp_generate(debwt_ctx *ctx);
/* Replaces sortBlue (src/sortBlue.c:10-57). */
int debwt_blue_sort(debwt_ctx *ctx);
/* Replaces insertCase3 up to the file writes (src/insertCase3.c:13-104). */
int debwt_bwt_assemble(debwt_ctx *ctx);

/* All five stages back to back (src/main.c:83-149). */
int debwt_build(debwt_ctx *ctx);

/* Copies the result to host memory: bwt ceil(n/32) words, hash_rows nrec-1 rows ascending,
 * dollar_row 1 row -- the contents of OUT, OUT.#, OUT.$ (src/insertCase3.c:115-131). */
int debwt_fetch_bwt(debwt_ctx *ctx, uint64_t *bwt, uint64_t *hash_rows, uint64_t *dollar_row);
/* debwt_build + debwt_fetch_bwt in one call, with the copy hidden behind the build: the reference writes OUT only after
 * its last stage (src/insertCase3.c:115-131); here a text that is built in several key ranges has the rows of a range
 * assembled as soon as the range's blocks are sorted, and they travel to `bwt` (page-locked memory for the overlap,
 * debwt_pinned_alloc) while the blocks of the next range are sorted.  Same buffers and contents as debwt_fetch_bwt. */
int debwt_build_to_host(debwt_ctx *ctx, uint64_t *bwt, uint64_t *hash_rows, uint64_t *dollar_row);
/* Only the row lists (OUT.#, OUT.$) -- for callers that keep the BWT words in HBM. */
int debwt_fetch_rows(debwt_ctx *ctx, uint64_t *hash_rows, uint64_t *dollar_row);
/* Device address of the packed BWT words of the last run (for callers that keep it in HBM). */
int debwt_bwt_device_ptr(debwt_ctx *ctx, const uint64_t **d_words);

/* Symbol census of the result in HBM: counts[c] = rows of the packed BWT that hold code c ('#' and '$' rows are
 * stored as 3, src/insertCase3.c:86-97) -- a BWT is a permutation of its text, so the census must equal the text's. */
int debwt_bwt_census(debwt_ctx *ctx, uint64_t counts[4]);

int debwt_get_stats(const debwt_ctx *ctx, debwt_stats *out);

/* Page-locked host memory for the text handed to debwt_load_text and the buffers debwt_fetch_bwt fills: the copies
 * then run at link rate and asynchronously (the reference keeps both in ordinary heap memory, src/collect#$.c:61,
 * src/insertCase3.c:115-119; pageable buffers work here too, only slower). */
int debwt_pinned_alloc(size_t bytes, void **out);
void debwt_pinned_free(void *p);

/* ---- one build over several GPUs: k-mer-prefix shards ----------------------------------
 * The reference has no distributed path; these entry points extend the stage sequence above for the case
 * that one text is built by `world` contexts (one per GPU, each holding the whole 2-bit text).  Shard r sorts
 * and classifies the keys of one prefix range -- in several key ranges one after the other when they do not
 * fit HBM at once -- and owns the BWT rows and the multi-in blocks of those nodes.
 * The collectives (bracketed) are the caller's (debwt_amd/sharded.py uses torch.distributed: RCCL or gloo).
 *
 * The keys reach their shard in one of two ways (debwt_shard_key_mode picks; everything after the sort is the same):
 * Key exchange (every shard scans only its 1/world slice of the text and ships 8-byte keys):
 *   load -> shard_begin -> shard_histogram -> [all-gather of the slice censuses] -> shard_plan(exchange = 1) ->
 *   shard_ranges -> [all-gather of the range cuts] -> shard_sort_begin ->
 *   per exchange round t:  shard_partition_keys (keys of the slice that fall into round t's ranges, grouped by owner)
 *                          -> [alltoallv of 8-byte keys: the k-mer bucket exchange] -> shard_sort_range(t) ->
 *   shard_sort_end -> ...
 * Key rescan (every shard holds the text anyway: it reads all of it once per key range and keeps its own keys --
 * n/4 bytes from its HBM instead of 8 n / world bytes from the fabric):
 *   ... -> shard_plan(exchange = 2) -> kmer_sort_rle -> ...
 * Then, sliced again (per-GPU work O(n / world)):
 *   shard_classify_local -> shard_facts_export -> [all-gather of the fact lists] ->
 *   shard_classify_global -> shard_sp_flags -> [all-gather of the slice SP lengths] -> shard_sp_emit ->
 *   [all-gather of the slice SP symbols] -> shard_sp_import -> shard_blue_route -> [alltoallv of 8-byte blue entries]
 *   -> shard_blue_place -> blue_sort -> bwt_assemble -> shard_info -> [gather of the packed row ranges] -> concat_rows.
 * Scan mode (no bulk exchange at all: tests and 2-GPU hosts without peer access):
 *   ... shard_plan(exchange = 0) or shard_set_range -> kmer_sort_rle -> shard_classify_local -> ... ->
 *   shard_classify_global -> sp_generate -> blue_sort -> bwt_assemble. */
#define DEBWT_KEYS_EXCHANGE 0
#define DEBWT_KEYS_RESCAN 1
/* Cost model of the two key paths for n text positions on `world` GPUs that each hold the text; link_gbytes_per_s:
 * sustained rate of one GPU-to-GPU link in one direction (<= 0: 48, i.e. 5/8 of an xGMI link's 76.8 GB/s).
 * Returns DEBWT_KEYS_EXCHANGE or DEBWT_KEYS_RESCAN, the estimated per-GPU milliseconds in *exchange_ms, *rescan_ms
 * (either may be NULL).  The constants are measured ones, see DESIGN.md section 7. */
int debwt_shard_key_mode(uint64_t n, int world, double link_gbytes_per_s, double *exchange_ms, double *rescan_ms);
int debwt_shard_begin(debwt_ctx *ctx, int rank, int world);           /* world <= 255 */
/* counts of this shard's slice of text positions by the top 12 bits of their key: 4096 words (host) */
int debwt_shard_histogram(debwt_ctx *ctx, uint64_t *hist4096);
/* this shard takes the keys whose top 12 bits lie in [bin_lo, bin_hi) as ONE key range: m_keys of them (from the
 * summed histogram), m_base keys in the shards before it */
int debwt_shard_set_range(debwt_ctx *ctx, uint32_t bin_lo, uint32_t bin_hi, uint64_t m_keys, uint64_t m_base);
/* the same from the summed census hist4096 (host), cut into as many key ranges as the free HBM (or debwt_set_range_cap)
 * asks for: the reference's segCount balancing (src/mySort.c:104-110) applied twice, over GPUs and over rounds.
 * exchange: 1 = the keys of every range will arrive through debwt_shard_sort_range; 0 = the shard reads them from
 * its text (debwt_kmer_sort_rle); 2 = the same with a sliced SP stage whose blue-entry exchange runs in the key buffers
 * (debwt_shard_scratch).  caller_held_bytes: device memory the caller already holds for
 * the exchanges of this build (counted as available: it is reused). */
int debwt_shard_plan(debwt_ctx *ctx, const uint64_t *hist4096, uint32_t bin_lo, uint32_t bin_hi, uint64_t m_base,
                     int exchange, uint64_t caller_held_bytes, uint32_t *nranges);
/* the cuts of debwt_shard_plan: range i = bins [bin_bounds[i], bin_bounds[i+1]) with m_keys[i] keys */
int debwt_shard_ranges(debwt_ctx *ctx, uint32_t *bin_bounds, uint64_t *m_keys, uint32_t capacity);
/* exchange mode: shard_of_bin: 4096 bytes (host), owner of each 12-bit prefix bin in this round, 0xFF = the bin is
 * not exchanged in this round; d_out: DEVICE buffer of `capacity` words; offs: world+1 host words,
 * group i = d_out[offs[i] .. offs[i+1]). */
int debwt_shard_partition_keys(debwt_ctx *ctx, const uint8_t *shard_of_bin, uint64_t *d_out, uint64_t capacity,
                               uint64_t *offs);
int debwt_shard_sort_begin(debwt_ctx *ctx);
/* d_keys: the `count` keys of range `range` in a DEVICE buffer the caller owns; it is used as sort workspace and must
 * stay untouched until the next shard_sort_range / shard_sort_end */
int debwt_shard_sort_range(debwt_ctx *ctx, uint32_t range, uint64_t *d_keys, uint64_t count);
int debwt_shard_sort_end(debwt_ctx *ctx);
int debwt_shard_classify_local(debwt_ctx *ctx, uint64_t *nfacts, uint64_t *nblocks, uint64_t *blue_rows);
/* copies the shard's nfacts fact words (node<<2 | 1 multi-out, | 2 multi-in) to a DEVICE buffer */
int debwt_shard_facts_export(debwt_ctx *ctx, uint64_t *d_dst, uint64_t capacity);
/* d_facts: DEVICE buffer with the facts of all shards (any order); qbase: blocks owned by the shards before
 * this one; blue_total: sum of blue_rows over all shards */
int debwt_shard_classify_global(debwt_ctx *ctx, const uint64_t *d_facts, uint64_t nfacts, uint64_t qbase,
                                uint64_t blue_total);
int debwt_shard_sp_flags(debwt_ctx *ctx, uint64_t *sp_symbols, uint64_t *mi_positions);
int debwt_shard_sp_emit(debwt_ctx *ctx, uint64_t sp_offset, uint8_t *d_dst, uint64_t capacity);
int debwt_shard_sp_import(debwt_ctx *ctx, const uint8_t *d_src, uint64_t sp_total);
/* first_block_of_shard: world+1 host words (exclusive scan of the shards' block counts) */
int debwt_shard_blue_route(debwt_ctx *ctx, const uint32_t *first_block_of_shard, uint64_t *d_out, uint64_t capacity,
                           uint64_t *offs);
/* Exchange buffers without an allocation: after the sort stage of a shard whose keys were read off the text (plan mode 0
 * or 2) its two key buffers are free until the next build.  DEBWT_SCRATCH_SEND: the buffer to route into
 * (debwt_shard_blue_route's d_out; the peers read it during the exchange); DEBWT_SCRATCH_RECV: the buffer to receive into
 * (debwt_shard_blue_place's d_entries) -- it holds the routed entries of the slice until debwt_shard_blue_route has run,
 * so it may be written only after that call.  *bytes = 0: none (keys exchanged: the receive buffer is the caller's own).
 * A host uses a scratch buffer when it is large enough and its own allocation otherwise; debwt_shard_plan mode 2 leaves
 * no room for exchange buffers beside the key buffers. */
#define DEBWT_SCRATCH_SEND 0
#define DEBWT_SCRATCH_RECV 1
int debwt_shard_scratch(debwt_ctx *ctx, int which, void **d_ptr, uint64_t *bytes);
/* d_entries: the `count` routed entries this shard received (DEVICE); the buffer is used as scratch and holds nothing
 * meaningful afterwards */
int debwt_shard_blue_place(debwt_ctx *ctx, uint64_t *d_entries, uint64_t count);
/* Final concat on one GPU: d_parts holds the shards' packed row ranges (part i from word part_word_off[i], one spare
 * word behind each, rows [row_base[i], row_base[i] + rows[i])); the ranges are not 32-row aligned and are
 * shift-merged into d_out (ceil(n/32) DEVICE words), as src/generateSP.c:379-405 joins SP segments. */
int debwt_concat_rows(debwt_ctx *ctx, const uint64_t *d_parts, uint32_t nparts, const uint64_t *part_word_off,
                      const uint64_t *row_base, const uint64_t *rows, uint64_t n, uint64_t *d_out);

/* first global row of the shard, its row count, and (after assemble) its number of '#' rows */
int debwt_shard_info(debwt_ctx *ctx, uint64_t *row_base, uint64_t *rows, uint64_t *hash_rows);
/* shard result to host: ceil(rows/32) words packed from the shard's first row (words may be NULL: row lists only);
 * GLOBAL '#' rows; the GLOBAL '$' row or ~0 when it is not in this shard */
int debwt_shard_fetch(debwt_ctx *ctx, uint64_t *words, uint64_t *hash_rows, uint64_t *dollar_row);

/* the shard's packed rows into a DEVICE buffer of `capacity` words (zero-filled behind the last row) */
int debwt_shard_export(debwt_ctx *ctx, uint64_t *d_words, uint64_t capacity);
/* debwt_bwt_census over any packed rows in HBM (n rows at d_words) */
int debwt_census_words(debwt_ctx *ctx, const uint64_t *d_words, uint64_t n, uint64_t counts[4]);

/* ---- the same build from ONE host process: one host thread per GPU, exchanges as peer-to-peer copies over xGMI --------
 * What the reference's single process with its thread pool (src/main.c:30) becomes on a node of GPUs: debwt_multi_build
 * runs the sharded stage sequence above (keys exchanged or rescanned) on `ngpus` contexts (devices[i] = HIP ordinal of shard i; NULL = 0, 1, ...;
 * ordinals may repeat -- several shards on one GPU -- which is how the path is tested on a one-GPU box), every shard
 * pulling its keys / facts / SP symbols / blue entries out of the other shards' buffers with device-to-device copies,
 * and leaves the concatenated BWT in the HBM of the first GPU.  cli/deBWT --gpus G is the C host on top of it. */
typedef struct debwt_multi debwt_multi;
typedef struct {
    uint64_t n, nrec;
    uint32_t ngpus, rounds;          /* exchange rounds = key ranges of the busiest shard */
    uint64_t key_bytes_in;           /* bytes of k-mers shard 0 pulled from the other shards (all rounds) */
    uint64_t blue_bytes_in;          /* bytes of blue entries shard 0 pulled from the other shards */
    float ms_build;                  /* wall time of debwt_multi_build */
    uint32_t key_mode;               /* DEBWT_KEYS_EXCHANGE or DEBWT_KEYS_RESCAN: how the keys reached their shards */
    uint32_t exchange_backend;       /* DEBWT_EXCHANGE_PEER_COPY or DEBWT_EXCHANGE_RCCL: what moved the data between the shards */
} debwt_multi_stats;
int debwt_multi_create(const debwt_config *cfg, const int *devices, int ngpus, debwt_multi **out);   /* cfg->device unused */
void debwt_multi_destroy(debwt_multi *m);
const char *debwt_multi_last_error(const debwt_multi *m);
debwt_ctx *debwt_multi_shard(debwt_multi *m, int shard);      /* the context of one shard (debwt_set_range_cap, stats) */
int debwt_multi_load_text(debwt_multi *m, const uint64_t *packed, uint64_t n, const uint64_t *sep, uint64_t nrec);
int debwt_multi_load_fasta(debwt_multi *m, const char *path, int threads, unsigned flags, uint64_t seed);
/* DEBWT_KEYS_EXCHANGE / DEBWT_KEYS_RESCAN, or -1 (the default): debwt_shard_key_mode decides at every build */
int debwt_multi_set_key_mode(debwt_multi *m, int key_mode);
/* What carries the exchanges between the shards (k-mer buckets, facts, SP symbols, blue entries, final row ranges):
 * DEBWT_EXCHANGE_PEER_COPY (default): every shard pulls its segments with device-to-device copies;
 * DEBWT_EXCHANGE_RCCL: one grouped ncclSend / ncclRecv alltoallv per exchange, one communicator per GPU of this process
 * (ncclCommInitAll; RCCL is loaded on demand -- DEBWT_EDEVICE where it is missing -- and needs one distinct GPU per shard).
 * The configured backend stays until this call changes it: when an RCCL exchange fails inside a build, every communicator
 * is aborted (the build returns the error), and the NEXT debwt_multi_build makes new communicators first -- or returns
 * DEBWT_EDEVICE with the reason in debwt_multi_last_error; it never falls back to peer copies by itself. */
#define DEBWT_EXCHANGE_PEER_COPY 0
#define DEBWT_EXCHANGE_RCCL 1
int debwt_multi_set_exchange(debwt_multi *m, int backend);
int debwt_multi_build(debwt_multi *m);
int debwt_multi_fetch_bwt(debwt_multi *m, uint64_t *bwt, uint64_t *hash_rows, uint64_t *dollar_row);
int debwt_multi_get_stats(const debwt_multi *m, debwt_multi_stats *out, debwt_stats *shard0);
/* What one shard of the last debwt_multi_build did, step by step -- the evidence for load balance over the shards (the
 * reference balances its per-thread segments by instance counts, src/mySort.c:104-110; whether that balances the later
 * stages too is a measurement).  ms[i]: wall milliseconds of step i (debwt_multi_step_name(i): the debwt_shard_* calls of
 * the sequence above, the exchanges, and "waiting" = time at the barriers between the stages, i.e. what the slowest
 * shard costs this one); bytes_in / bytes_out: what the shard received from / sent to OTHER shards in each exchange
 * (0 keys, 1 facts, 2 SP symbols, 3 blue entries, 4 final rows).
 * debwt_multi_set_serial(m, 1): the shards of a build take turns between the barriers, one on its GPU at a time, device
 * drained around every step -- the steps' times are then each shard's own even when several shards share one GPU (the
 * way N = 2, 4, 8 are measured on a one-GPU box; peer-copy exchanges only).  The result of the build is the same. */
#define DEBWT_MULTI_STEPS 24
typedef struct {
    float ms[DEBWT_MULTI_STEPS];
    uint64_t bytes_in[5], bytes_out[5];
    uint64_t keys, key_ranges, blocks, blue_rows, rows;   /* node instances, key ranges, multi-in blocks, their rows, BWT rows */
    uint32_t bin_lo, bin_hi;                              /* the shard's 12-bit prefix bins [bin_lo, bin_hi) */
} debwt_shard_report;
int debwt_multi_set_serial(debwt_multi *m, int serial);
int debwt_multi_get_shard_report(const debwt_multi *m, int shard, debwt_shard_report *out);
const char *debwt_multi_step_name(int step);

/* ---- intermediates, for stage-by-stage parity ---------------------------------- */
typedef enum {
    DEBWT_ARR_SORTED_KEYS = 1, /* u64 x n_main: (node<<2|pred) ascending; after debwt_kmer_sort_rle of a one-range
                                  build driven stage by stage on one GPU only (debwt_build and shards keep the
                                  run-length encoding alone: DEBWT_ESTATE, as in a build of several key ranges)    */
    DEBWT_ARR_DISTINCT_KEYS,   /* u64 x distinct_keys                                                 */
    DEBWT_ARR_RED,             /* u64 x red_capacity: node<<2 | multiin<<1 | multiout, ascending      */
    DEBWT_ARR_SP_SYMBOLS,      /* u8  x sp_len: SP symbols 0..5                                       */
    DEBWT_ARR_BLUE,            /* u64 x blue_capacity: pred | spIndex<<4 (src/generateSP.c:666-672)   */
    DEBWT_ARR_BLUE_BOUND,      /* u64 x blue_bound_num: inclusive end of each block (blueBound)       */
    DEBWT_ARR_CASE3_BOUND,     /* u64 x case3num: [first row,last row] per block (case3bound)         */
    DEBWT_ARR_ROW_SYMBOLS      /* u8  x n: BWT symbols 0..5 by row (after assemble)                   */
} debwt_array;
/* Copies up to `capacity` elements; *count receives the element count of the array. */
int debwt_fetch_array(debwt_ctx *ctx, debwt_array which, void *dst, uint64_t capacity, uint64_t *count);

/* The same intermediates written as files in the byte formats of the reference's own temp files and global arrays, so
 * that a build can be bisected stage by stage against the reference (cli/deBWT --dump DIR drives this; the names are the
 * reference's, `oracle/_ref/ref_driver` in the build container writes the same set as OUT.<name>):
 *   DEBWT_DUMP_KMERINFO  any time after the load (runs debwt_kmer_count_sorted: the pipeline is back at "text loaded"):
 *                        kmerInfo = D x {u64 k-mer left-aligned, u64 count} (src/mySort.c:193-195);
 *   DEBWT_DUMP_BLOCKS    after debwt_classify: redSeq, redPoint (src/INandOut.c:396-405), blueBound (:359-361),
 *                        case3bound (:347-353), raw u64 arrays;
 *   DEBWT_DUMP_SP        after debwt_sp_generate, before debwt_blue_sort: spCode (ceil(S / 32) words, 2 bits per symbol,
 *                        separators as 3; src/generateSP.c:626-660), spSpecialIndex (N x u64, :630-641), blueTable
 *                        (B x u64 pred | spIndex << 4, :666-672; the order INSIDE a block is the arrival order of the
 *                        scan -- thread-dependent in the reference too -- only the set per block is defined).
 * One-range builds driven stage by stage on one GPU (as debwt_fetch_array).  DEBWT_EIO: dir missing or not writable. */
#define DEBWT_DUMP_KMERINFO 1
#define DEBWT_DUMP_BLOCKS 2
#define DEBWT_DUMP_SP 3
int debwt_dump_reference_files(debwt_ctx *ctx, const char *dir, int stage);

/* ---- primitives exposed for measurement and parity ------------------------------------------- */

/* Stand-alone a-1+a-2 in the reference's own output format: every k-mer inside a record,
 * sorted ascending, left-aligned, with its count -- the contents of `kmerInfo`
 * (src/mySort.c:193-195).  Needs a loaded text.  kmers/counts: host arrays of `capacity`
 * entries; *distinct receives D. */
int debwt_kmer_count_sorted(debwt_ctx *ctx, uint64_t *kmers, uint64_t *counts, uint64_t capacity,
                            uint64_t *distinct);

/* LSD radix sort of `count` 64-bit keys resident in HBM (d_keys, d_tmp: device pointers, both
 * `count` words; result in d_keys).  key_bits: significant low bits (1..64); every key must be below 2^key_bits -- the
 * bucket finish relies on it (bits above key_bits are not ignored: with them the result is undefined, not merely misordered).
 * ms_per_pass (optional) receives the mean device time of one scatter pass. */
int debwt_radix_sort_u64(debwt_ctx *ctx, uint64_t *d_keys, uint64_t *d_tmp, uint64_t count, int key_bits,
                         float *ms_per_pass);
/* The same for keys the caller knows to lie in [key_lo, key_hi) (key_hi = 0: no upper bound), as the keys of one key
 * range of a build do: when the top byte of such keys takes few values, the last pass takes its chunk histograms from
 * the count kernel of the pass before it.  DEBWT_EINVAL when a key lies outside the bounds (nothing is sorted then). */
int debwt_radix_sort_u64_range(debwt_ctx *ctx, uint64_t *d_keys, uint64_t *d_tmp, uint64_t count, int key_bits,
                               uint64_t key_lo, uint64_t key_hi, float *ms_per_pass);
/* Passes this process has run that took their chunk histograms from the pass before them (tests and A/B runs: which form
 * a sort took; DEBWT_HIST_EVERY_PASS=1 in the environment keeps it from counting up). */
uint64_t debwt_radix_pair_passes(void);
/* Sorts this process has run whose lowest prefix digit was split bucket by bucket in LDS (one streaming pass) instead of by
 * a count and a scatter pass in HBM.  By default that is the key ranges of four prefix digits; DEBWT_BUCKET_PASS=0 in the
 * environment restores the HBM pass everywhere, DEBWT_BUCKET_PASS=1 takes the bucket pass in every sort with a bucket
 * finish and gives every sort at least two prefix digits (tests: small inputs reach it). */
uint64_t debwt_radix_bucket_passes(void);
/* Sorts this process has run whose bucket finish took its low-word form (prefix buckets cut at bit 32 or below: only the low
 * words of a wave tile are exchanged).  DEBWT_FINISH_LOW=0 in the environment keeps whole keys everywhere and this from
 * counting up; DEBWT_PREFIX_DIGITS=<1..4> forces the number of prefix digits of every sort (tests: small inputs reach it). */
uint64_t debwt_radix_low_finishes(void);

/* Host-only: checksums of the special-region tables (`collect`'s specialSA / specialBwt / specialBranch / head / tail
 * tables, src/collect#$.c:118-157,348-602) that debwt_kmer_sort_rle builds on host threads for the loaded text layout;
 * digest[0..3] = order of the special suffixes, their keys + BWT symbols, the special branches, the head/tail nodes.
 * Lets tests compare the threaded module with its single-threaded run (DEBWT_SPECIAL_THREADS / DEBWT_SPECIAL_PAR_MIN). */
int debwt_special_digest(const uint64_t *packed, uint64_t n, const uint64_t *sep, uint64_t nrec, int k, uint64_t digest[4]);

/* Needs a GPU and a loaded text: builds the same tables on the device (the path collections of many records take,
 * SURVEY 8f-1) and by the host module, and counts the elements that differ: mismatch[0..5] = suffix order of the
 * special suffixes, their keys, their BWT symbols, the special branches, the head nodes, the tail nodes.  A build in
 * progress is discarded (the context is back at "text loaded"); the counters of the last build are left alone. */
int debwt_special_compare(debwt_ctx *ctx, uint64_t mismatch[6]);

/* Verification tool standing in for the dead LFsearch path (src/LFsearch.c:14-48): inverse BWT
 * by LF walk on the host from a fetched result; writes the n symbols (0..5).  Returns 0 when the
 * walk closes; DEBWT_EINVAL for row lists or listed rows that debwt_verify_device refuses (below). */
int debwt_verify_inverse(const uint64_t *bwt, uint64_t n, const uint64_t *hash_rows, uint64_t nrec,
                         uint64_t dollar_row, uint8_t *sym_out);

/* The same check on the device, for results that never leave HBM and for sizes where one chain of n dependent LF steps
 * (the reference's walk, src/LFsearch.c:49-166, ~0.2 us per step on a host core) takes hours: a sampled rank structure
 * over the packed rows (the reference's occ tables, src/insertCase3.c:141-194, as one 128-byte line per 384 rows), the
 * rows of ~`segments` text positions found by backward search of the text in the BWT, and one LF walk per segment, each
 * compared symbol by symbol with the loaded text and required to end on the row the previous segment starts from --
 * together one chain over all n rows.  d_words: DEVICE packed rows (NULL: the context's own result, with its row
 * lists); hash_rows / dollar_row: OUT.# / OUT.$ (host).  segments 0 = default.  ok = 1: the inverse BWT of the rows is
 * the loaded text.
 * Refused with DEBWT_EINVAL and a reason in debwt_last_error, before any search or walk (debwt_fm_create and
 * debwt_fm_open make the same checks):
 *   - dollar_row >= n, or a '#' row >= n;
 *   - '#' rows that are not strictly ascending (descending or repeated rows);
 *   - the '$' row among the '#' rows;
 *   - a '#' row or the '$' row whose stored code is not 3 (the format puts code 3 under both, see debwt_bwt_census);
 *   - a census with fewer code-3 rows than records.
 * Rows that pass are walked with a C[] table taken from their own census, so every LF step stays inside [0, n)
 * whatever the rows hold; bits of the last word beyond row n - 1 are never read as rows. */
typedef struct {
    uint64_t segments, steps, mismatches, broken_links, search_failures, search_steps;
    float ms_index, ms_search, ms_walk;
    int ok;
} debwt_verify_report;
int debwt_verify_device(debwt_ctx *ctx, const uint64_t *d_words, const uint64_t *hash_rows, uint64_t dollar_row,
                        uint64_t segments, debwt_verify_report *report);
/* the same on the concatenated result of debwt_multi_build (first GPU; every GPU holds the text) */
int debwt_multi_verify(debwt_multi *m, debwt_verify_report *report);

/* FM-index over built rows: the verifier's rank structure (one 128-byte line per 384 rows), a suffix array sampled every
 * sa_sample rows (a power of two in 1..1024, 0 = 32; one u64 text position per sample), batched count (one backward
 * search per pattern) and locate (one LF walk per occurrence to the nearest sampled row: s steps expected, not bounded).
 * An index owns its device memory and its stream; it is not re-entrant. */
typedef struct debwt_fm debwt_fm;
typedef struct {
    uint64_t n, nrec, sa_sample, samples, device_bytes;
    float ms_rank, ms_samples;
    uint64_t census[4];      /* rows per 2-bit code, '#' and '$' rows counted as 3 (as debwt_bwt_census) */
} debwt_fm_info;
/* ctx: a text loaded.  rows NULL: the context's own result (after a build); else HOST packed rows (OUT) with hash_rows
 * (OUT.#, nrec - 1 rows) and dollar_row (OUT.$).  The samples come from the verifier's walk over the loaded text, so an
 * index is made only of rows that are the BWT of that text: otherwise DEBWT_EINVAL with the reason in debwt_last_error.
 * The index outlives the context. */
int debwt_fm_create(debwt_ctx *ctx, const uint64_t *rows, const uint64_t *hash_rows, uint64_t dollar_row,
                    uint32_t sa_sample, debwt_fm **out);
/* the same index from saved files alone (no text): rows of n symbols, nrec - 1 '#' rows, the '$' row and the
 * ceil(n / sa_sample) samples debwt_fm_samples returned.  The rows are not checked against a text. */
int debwt_fm_open(int device, const uint64_t *rows, uint64_t n, const uint64_t *hash_rows, uint64_t nrec,
                  uint64_t dollar_row, const uint64_t *samples, uint32_t sa_sample, debwt_fm **out);
const char *debwt_fm_last_error(const debwt_fm *fm);
int debwt_fm_info_get(const debwt_fm *fm, debwt_fm_info *out);
/* the samples (info.samples words) and the first text position of every record (nrec words, ascending) */
int debwt_fm_samples(debwt_fm *fm, uint64_t *dst, uint64_t capacity);
int debwt_fm_record_starts(const debwt_fm *fm, uint64_t *dst, uint64_t capacity);
/* patterns: ASCII concatenated, pattern i = patterns[offsets[i] .. offsets[i + 1]).  ranges[2i] = lo, ranges[2i + 1] = hi:
 * the rows of the suffixes that start with pattern i, count = hi - lo.  A/C/G/T in either case; an empty pattern or one
 * with any other character occurs 0 times.  Large batches are cut inside. */
int debwt_fm_count(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat, uint64_t *ranges);
/* ranges as debwt_fm_count wrote them.  out_offsets (npat + 1): prefix sums of min(hi - lo, max_per_pattern);
 * positions[out_offsets[i] ..]: the global text positions of pattern i's first rows, in row order.  DEBWT_ERANGE when
 * capacity is below out_offsets[npat] (out_offsets is written first).  max_per_pattern 0 = no cap. */
int debwt_fm_locate(debwt_fm *fm, const uint64_t *ranges, uint64_t npat, uint64_t max_per_pattern,
                    uint64_t *out_offsets, uint64_t *positions, uint64_t capacity);
/* Search with up to max_mismatches (0..4) substitutions among A/C/G/T.  A hit is one distinct text string W, |W| = |P|,
 * Hamming(W, P) <= K, W inside one record; a pattern character outside ACGTacgt matches no base (one mismatch whatever
 * the text holds).  K = 0 agrees with debwt_fm_count: 0 hits, or 1 hit with count's [lo, hi).  An empty pattern has 0
 * hits; a pattern longer than 1024 bytes or K > 4 is DEBWT_EINVAL.  DEBWT_FM_BOTH_STRANDS also searches the reverse
 * complement (A<->T, C<->G; other characters stay mismatch characters), hits of strand 1.  DEBWT_FM_BEST_ONLY keeps per
 * pattern only the hits of the smallest mismatch count, over both strands when both are searched (searched stratum by
 * stratum, so deeper strata are not explored once a pattern has hits).
 * hit_offsets (npat + 1): pattern i's hits are [hit_offsets[i], hit_offsets[i+1]), ascending by (strand, mismatches,
 * lo).  ranges: 2 words per hit, the same layout debwt_fm_count writes, so they can go straight into debwt_fm_locate
 * (one "pattern" per hit).  hit_info: per hit, mismatches in bits 0-7, strand in bit 8 (0 forward, 1 reverse
 * complement).  DEBWT_ERANGE when capacity < hit_offsets[npat]; hit_offsets is written first (same protocol as
 * debwt_fm_locate).  Device scratch is capped: (K + 1) buffers of DEBWT_FM_SEARCH_ITEMS (environment, read per call;
 * default 2^23) items of 24 bytes, at most 960 MiB. */
#define DEBWT_FM_BOTH_STRANDS 1u
#define DEBWT_FM_BEST_ONLY    2u
int debwt_fm_search(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                    uint32_t max_mismatches, uint32_t flags,
                    uint64_t *hit_offsets, uint64_t *ranges, uint32_t *hit_info, uint64_t capacity);
/* what the last debwt_fm_search did: work items per level (level 0: pattern x strand searches, per stratum with
 * DEBWT_FM_BEST_ONLY), rank steps (one fm_occ4 each), rank lines read, kernel launches and the launches re-run in smaller
 * chunks after a buffer overflowed, hits before the final sort, kernel time (events) and host wall time */
typedef struct {
    uint64_t patterns, batches, launches, retries, hits, steps, line_reads, scratch_bytes;
    uint64_t items[5];
    float ms_kernel, ms_wall;
} debwt_fm_search_stats;
int debwt_fm_search_stats_get(const debwt_fm *fm, debwt_fm_search_stats *out);
/* Maximal exact matches of each pattern (and of its reverse complement with DEBWT_FM_BOTH_STRANDS) of length >= min_len
 * (>= 1).  With s(e) the smallest s such that P[s..e] occurs inside one record (e + 1 when P[e] is outside ACGTacgt or
 * does not occur), the MEMs are the spans [s(e), e + 1) with s(e) <= e where e = m - 1 or s(e + 1) > s(e): they occur and
 * cannot be extended by one base on either side.  Exact, with no cap; any pattern length below 2^32 bytes, an empty
 * pattern has 0 MEMs.
 * mem_offsets (npat + 1): pattern i's MEMs are [mem_offsets[i], mem_offsets[i+1]), ascending by (strand, qbeg).
 * spans: 2 u32 per MEM, [qbeg, qend) in the coordinates of the pattern AS GIVEN, also for strand 1 (the text there
 * reads revcomp(P[qbeg..qend))).  ranges: 2 u64 per MEM, the debwt_fm_count layout (straight into debwt_fm_locate).
 * strands: 1 byte per MEM.  DEBWT_ERANGE when capacity < mem_offsets[npat], mem_offsets written first.  DEBWT_EINVAL for
 * min_len 0, flags other than DEBWT_FM_BOTH_STRANDS, decreasing offsets and a pattern of 2^32 bytes or more.
 * Batches are cut inside the library at 64 MB of pattern bytes and DEBWT_FM_MEM_SLOTS (environment, read per call;
 * default 2^24) worst-case MEM slots, max(0, m - min_len + 1) per pattern and strand; a pattern with more goes alone.
 * Device scratch: 24 bytes per slot, 24 per MEM found, 20 per pattern and strand and the pattern bytes, each with up to
 * 25 % slack: at most about 1.2 GB at the default (more only for a single pattern beyond the slot limit). */
int debwt_fm_mems(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat, uint32_t min_len,
                  uint32_t flags, uint64_t *mem_offsets, uint32_t *spans, uint64_t *ranges, uint8_t *strands,
                  uint64_t capacity);
/* what the last debwt_fm_mems did: patterns, batches, kernel launches (k_fm_mems and the compaction), MEMs, rank steps
 * (one fm_occ2 each), rank lines read, wave steps (64 x the longest lane per wave: steps / wave_steps is the share of
 * lanes busy), the largest slot scratch of a batch, k_fm_mems time (events) and host wall time */
typedef struct {
    uint64_t patterns, batches, launches, mems, steps, line_reads, wave_steps, scratch_bytes;
    float ms_kernel, ms_wall;
} debwt_fm_mems_stats;
int debwt_fm_mems_stats_get(const debwt_fm *fm, debwt_fm_mems_stats *out);

/* ---- suffix-prefix overlaps of patterns against the records (fm_overlap_kernels.h) --------------------------------
 * For every pattern, the records whose beginning equals its end.  Q is the pattern as given (strand 0) or, with
 * DEBWT_FM_BOTH_STRANDS, also its reverse complement (strand 1; complementing as in debwt_fm_mems: A<->T, C<->G, other
 * characters stay non-bases).  With m = |Q| and S_j the string of record j, (Q, j, L) is an overlap iff
 *   min_overlap <= L <= min(m, |S_j|),  Q[m-L .. m) == S_j[0 .. L) with A/C/G/T in either case,  and all of Q[m-L .. m)
 *   are bases.
 * A character outside ACGTacgt at Q[p] therefore limits L to m - 1 - p, and one at Q[m-1] gives no overlap.  EVERY overlap
 * is reported: the overlap of a record of the collection with itself (L = m = |S_j|), containments, and several lengths
 * with one record (periodic reads).  Exact overlaps only; debwt_fm_overlaps_mm below takes a mismatch budget.
 * A hit is (record j, length L, strand, flags): DEBWT_FM_OVERLAP_CONTAINS when L == |S_j| (the record is a suffix of Q),
 * DEBWT_FM_OVERLAP_WHOLE when L == m (Q is a prefix of the record).
 * Strand 1, read carefully: a strand-1 hit says that the last L bases of revcomp(P) start record j, that is, record j
 * begins with the reverse complement of P's FIRST L bases.  On a collection that holds reads of one strand only this
 * finds head-to-head overlaps; tail-to-tail ones (a read's end against the reverse complement of another read's end) need
 * the reverse complements in the collection (or an index of the reversed text) and are not found here.
 * hit_offsets (npat + 1): pattern i's hits are [hit_offsets[i], hit_offsets[i+1]), ascending by (strand, length
 * DESCENDING, record ascending): an order the strings alone determine, whatever order the BWT gives equal suffixes.
 * An empty pattern has 0 hits, as has one shorter than min_overlap; pattern length below 2^32 bytes; fewer than 2^32
 * records.  DEBWT_ERANGE when capacity < hit_offsets[npat], hit_offsets written first (the protocol of debwt_fm_locate).
 * DEBWT_EINVAL for min_overlap 0, flags other than DEBWT_FM_BOTH_STRANDS | DEBWT_FM_OVERLAP_LONGEST, decreasing offsets
 * and a pattern of 2^32 bytes or more.  No attached text is needed: an index from debwt_fm_open answers as one from
 * debwt_fm_create.
 * DEBWT_FM_OVERLAP_LONGEST keeps per (pattern, strand, record) only the largest L: a subsequence of the full result, bit
 * for bit what debwt_fm_overlap_longest makes of it (capacity then counts the kept hits).  With this flag a NULL hits
 * never fits: a call without any hit and with hits NULL answers DEBWT_ERANGE (hit_offsets[npat] = 0), and DEBWT_OK without
 * the flag; debwt_fm_overlaps_mm does the same.
 * The first call makes the record table (for every separator row the record that starts there and its length, 8 bytes
 * per record, from a locate of the '#' suffixes: DEBWT_EINTERNAL if one does not land on a record start) and keeps it
 * with the index: it is counted in debwt_fm_info.device_bytes from then on.
 * Batches are cut inside the library at 64 MB of pattern bytes, 2^20 patterns and DEBWT_FM_OVERLAP_SLOTS (environment,
 * read per call; default 2^24) worst-case run slots, max(0, m - min_overlap + 1) per pattern and strand; a pattern with
 * more goes alone.  Hits are expanded at most DEBWT_FM_OVERLAP_HITS (default 2^24) at a launch, from counts that are
 * exact after the walk, so there is no worst-case hit buffer; the result depends on neither limit.  Device scratch: 16
 * bytes per slot, 24 per run found, 16 per hit of one launch, 36 per pattern and strand and the pattern bytes, each with
 * up to 25 % slack: at most about 0.8 GB at the defaults (more only for a single pattern beyond the slot limit). */
#define DEBWT_FM_OVERLAP_LONGEST  2u   /* option flag, beside DEBWT_FM_BOTH_STRANDS (1u) */
#define DEBWT_FM_OVERLAP_CONTAINS 1u   /* hit flag: length == length of `record` (the record is a suffix of Q) */
#define DEBWT_FM_OVERLAP_WHOLE    2u   /* hit flag: length == |Q| (Q is a prefix of the record) */
typedef struct { uint32_t record, length, strand, flags; } debwt_fm_overlap;
int debwt_fm_overlaps(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                      uint32_t min_overlap, uint32_t flags,
                      uint64_t *hit_offsets, debwt_fm_overlap *hits, uint64_t capacity);
/* what the last debwt_fm_overlaps did: patterns, batches, kernel launches (walk, compaction, expansions), runs (one per
 * pattern, strand and length with at least one record), hits (hit_offsets[npat]), rank steps (one fm_occ2 each), rank
 * lines read, wave steps (64 x the longest lane per wave: steps / wave_steps is the share of lanes busy), the largest
 * scratch of a batch, kernel time (events; walk + compaction + expansion) and host wall time */
typedef struct {
    uint64_t patterns, batches, launches, runs, hits, steps, line_reads, wave_steps, scratch_bytes;
    float ms_kernel, ms_wall;
} debwt_fm_overlaps_stats;
int debwt_fm_overlaps_stats_get(const debwt_fm *fm, debwt_fm_overlaps_stats *out);
/* The reduction of DEBWT_FM_OVERLAP_LONGEST on the host (no GPU): hits in the order above, pattern i's in [offsets_in[i],
 * offsets_in[i+1]); per (pattern, strand, record) the first (longest) hit stays.  Compacts `hits` in place from
 * offsets_in[0] and writes the new offsets (npat + 1; offsets_out may be offsets_in).  DEBWT_EINVAL, with nothing moved,
 * when the input is not in that order (decreasing offsets, a strand above 1, strands descending, lengths ascending inside
 * a strand, records not strictly ascending inside a length). */
int debwt_fm_overlap_longest(debwt_fm_overlap *hits, const uint64_t *offsets_in, uint64_t npat, uint64_t *offsets_out);

/* ---- suffix-prefix overlaps with up to K mismatches (fm_overlap_mm_kernels.h) --------------------------------------
 * Q, strand, m and S_j as in debwt_fm_overlaps.  For min_overlap <= L <= min(m, |S_j|) let mm(Q, j, L) be the number of
 * columns c in [0, L) where Q[m-L+c] does not equal S_j[c] (A/C/G/T in either case; a character of Q outside ACGTacgt
 * equals no base: one mismatch whatever the record holds, the rule of debwt_fm_search).  (Q, j, L) is a hit iff
 *   mm <= max_mismatches  and  (max_error_permille == 0  or  1000 * mm <= max_error_permille * L).
 * Every hit is reported once: self overlaps, containments and several lengths of one record all appear, and a record can
 * appear at a length with mm > 0 next to a longer or shorter length with another mm.
 * A hit is the debwt_fm_overlap of debwt_fm_overlaps: flags bits 0-1 are DEBWT_FM_OVERLAP_CONTAINS / DEBWT_FM_OVERLAP_WHOLE,
 * bits 8-15 hold mm (DEBWT_FM_OVERLAP_MM).  The order per pattern is that of debwt_fm_overlaps, (strand, length DESCENDING,
 * record ascending); mm takes no part in it, and as a (record, length, strand) occurs once the order is total and
 * debwt_fm_overlap_longest accepts the list as it is.  DEBWT_FM_BOTH_STRANDS and DEBWT_FM_OVERLAP_LONGEST as there:
 * LONGEST keeps the largest L per (pattern, strand, record) whatever its mm, bit for bit what debwt_fm_overlap_longest
 * makes of the full list.  With max_mismatches 0 the result is that of debwt_fm_overlaps with the same arguments,
 * hit_offsets and every byte of hits.
 * max_mismatches 0..4, max_error_permille 0..1000 (0: no rate limit), a pattern of at most 1024 bytes, fewer than 2^31
 * patterns; otherwise, and for min_overlap 0, unknown flags and decreasing offsets, DEBWT_EINVAL with the reason in
 * debwt_fm_last_error.  An empty pattern, or one shorter than min_overlap, has 0 hits.  DEBWT_ERANGE as debwt_fm_overlaps:
 * hit_offsets is written first, the remaining batches are only counted.  No attached text is needed.
 * Batches are cut at 64 MB of pattern bytes and DEBWT_FM_OVERLAP_BATCH patterns (environment, read per call; default and
 * cap 2^20).  Device scratch is capped as in debwt_fm_search: one buffer of DEBWT_FM_OVERLAP_ITEMS (environment, read per
 * call; default 2^23, raised to at least 4 * 1024 + 64 so that a chunk of one item always fits) items of 24 bytes per
 * level 1..K and one of as many runs of 16 bytes, 0.94 GB at K = 4 and the default; beside them, as in
 * debwt_fm_overlaps, 24 bytes per run found in one batch, 16 per hit of one launch (at most DEBWT_FM_OVERLAP_HITS,
 * default 2^24) and the pattern bytes, each with up to 25 % slack.  The result depends on none of the limits. */
#define DEBWT_FM_OVERLAP_MM(flags) (((flags) >> 8) & 0xFFu)   /* mismatches of a hit of debwt_fm_overlaps_mm */
int debwt_fm_overlaps_mm(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                         uint32_t min_overlap, uint32_t max_mismatches, uint32_t max_error_permille, uint32_t flags,
                         uint64_t *hit_offsets, debwt_fm_overlap *hits, uint64_t capacity);
/* what the last debwt_fm_overlaps_mm did: patterns, batches, kernel launches (levels and expansions), the level launches
 * re-run in smaller chunks after a buffer overflowed, runs (one per work item and length with at least one record), hits
 * (hit_offsets[npat]), rank steps (one fm_occ4 each), rank lines read, wave steps (64 x the longest lane per wave), the
 * scratch this call may fill, work items per mismatch level, kernel time (events) and host wall time */
typedef struct {
    uint64_t patterns, batches, launches, retries, runs, hits, steps, line_reads, wave_steps, scratch_bytes;
    uint64_t items[5];          /* work items per mismatch level, as debwt_fm_search_stats */
    float ms_kernel, ms_wall;
} debwt_fm_overlaps_mm_stats;
int debwt_fm_overlaps_mm_stats_get(const debwt_fm *fm, debwt_fm_overlaps_mm_stats *out);

/* ---- gapped extension of seeds and a read mapper (fm_extend_kernels.h) -------------------------------------------
 * An index holds no text; the two entry points below read the text next to a seed, so it is attached first (n / 4 bytes
 * of HBM, counted in debwt_fm_info.device_bytes, as is the record table of debwt_fm_overlaps once made).  Without it they answer DEBWT_ESTATE; count, locate, search and mems
 * never need it.
 *   ctx given: device-to-device copy of the context's loaded text (same n and nrec, else DEBWT_EINVAL); packed / sep are
 *              ignored.  The path after debwt_fm_create.
 *   ctx NULL:  packed (host words in the format of debwt_load_text) and sep (the nrec separator positions) are uploaded.
 *              The path after debwt_fm_open; a host gets them from debwt_pack_fasta.
 * The text must be the index's text: the separators must be the record starts - 1 (and n - 1), and for every sample i
 * with p = sa[i] > 0 the 2-bit code of row i * sa_sample must be the text's code at p - 1 (checked on the device);
 * otherwise DEBWT_EINVAL with the reason in debwt_fm_last_error, and no text is attached.  debwt_fm_restore_text (below)
 * attaches the same text without a source, from the index alone. */
int debwt_fm_attach_text(debwt_fm *fm, debwt_ctx *ctx, const uint64_t *packed, const uint64_t *sep);

/* Banded affine-gap local alignment of jobs.  A job aligns the query string Q (length m, 1..65535) of pattern `pattern`
 * -- the pattern itself (strand 0) or its reverse complement (strand 1); a character outside ACGTacgt mismatches every
 * base -- against record `record` around the diagonal `diag` = text position - query position.  Scoring: match a > 0,
 * mismatch b > 0, gap open o >= 0, gap extend e > 0, each at most 255; a gap of length L costs o + L * e.  band: the
 * half-width w, 0..63.  With [rs, re) the text positions of the record's bases, a cell (i, t) is allowed iff
 * 0 <= i < m, rs <= t < re and |t - i - diag| <= w; over allowed cells, with -inf for every value at any other cell:
 *     E(i,t) = max(H(i,t-1) - o - e, E(i,t-1) - e)                  deletion: consumes text t
 *     F(i,t) = max(H(i-1,t) - o - e, F(i-1,t) - e)                  insertion: consumes query i
 *     H(i,t) = max(0 + s(i,t), H(i-1,t-1) + s(i,t), E(i,t), F(i,t)),   s = +a if Q[i] == T[t] else -b
 *     score  = max(0, max over allowed cells of H)
 * out[j]: score, and for score > 0 one optimal alignment: [qbeg, qend) IN Q -- for strand 1 these are coordinates of the
 * reverse complement, unlike the spans of debwt_fm_mems (which are in the pattern as given): a CIGAR reads left to right
 * along the text --, [tbeg, tend) global text positions, edits = mismatch columns + gap bases.  cigar_offsets (njobs + 1)
 * and cigar: job j's ops are cigar[cigar_offsets[j] .. cigar_offsets[j + 1]), BAM-coded (len << 4 | op, M 0, I 1, D 2);
 * DEBWT_ERANGE when capacity < cigar_offsets[njobs] (cigar_offsets and out are written first, as debwt_fm_locate does).
 * score 0: empty CIGAR, coordinates 0.  cigar_offsets NULL: score only -- no traceback is stored; qend and tend are the
 * end of the best alignment, qbeg = tbeg = edits = 0.
 * Among optimal alignments: the end cell is the one with the smallest query index, then the smallest text position; walking
 * back, H prefers the diagonal (and stops where H(i-1,t-1) <= 0) to E to F, and a gap is opened rather than continued on a
 * tie.  The result does not depend on how the jobs are batched.
 * DEBWT_EINVAL: band > 63, a scoring value out of range, a job with pattern >= npat, strand > 1, record >= nrec or a
 * pattern length outside 1..65535.  Device scratch: (2m + 2w - 1 or fewer) x (w + 1) flag bytes per job with a traceback;
 * batches are cut at DEBWT_FM_EXTEND_BYTES of it (environment, read per call; default 512 MiB; a job above it goes alone). */
typedef struct {
    uint64_t pattern;
    int64_t diag;
    uint32_t record, strand;
} debwt_fm_job;
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend;
} debwt_fm_scoring;
typedef struct {
    int32_t score;
    uint32_t qbeg, qend, edits;
    uint64_t tbeg, tend;
} debwt_fm_aln;
int debwt_fm_extend(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat, const debwt_fm_job *jobs,
                    uint64_t njobs, const debwt_fm_scoring *scoring, uint32_t band, debwt_fm_aln *out,
                    uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity);
/* what the last debwt_fm_extend (or the extension stage of the last debwt_fm_map) did: jobs, batches, kernel launches,
 * allowed cells computed, steps of the waves (one anti-diagonal each: cells / (64 x wave_steps) is the share of lanes
 * busy), the largest flag scratch of a batch, kernel time (events: sweep, traceback) and host wall time */
typedef struct {
    uint64_t jobs, batches, launches, cells, wave_steps, scratch_bytes;
    float ms_kernel, ms_trace, ms_wall;
} debwt_fm_extend_stats;
int debwt_fm_extend_stats_get(const debwt_fm *fm, debwt_fm_extend_stats *out);

/* Seeds of ONE read to extension candidates (host only, no GPU; the clustering step of debwt_fm_map).  A seed is an exact
 * match Q[qbeg, qend) = T[diag + qbeg, diag + qend) inside `record`.  Sorted by (strand, record, diag), a seed joins the
 * open cluster when strand and record agree and its diag is at most `band` above the diag of the cluster's first seed,
 * otherwise it opens a new one.  weight = distinct query positions the cluster's seeds cover.  The max_cand heaviest
 * clusters are written, heaviest first, ties by smaller (strand, record, first seed's diag).  A candidate's diag is that
 * of its longest seed (ties: smallest qbeg, then smallest diag).  Returns the number written (<= max_cand), or
 * DEBWT_EINVAL (a seed with qend <= qbeg). */
typedef struct {
    int64_t diag;
    uint32_t record, strand, qbeg, qend;
} debwt_fm_seed;
typedef struct {
    int64_t diag, first_diag;
    uint32_t record, strand, weight, seeds;
} debwt_fm_cand;
int debwt_fm_cluster_seeds(const debwt_fm_seed *seeds, uint64_t nseeds, uint32_t band, uint32_t max_cand,
                           debwt_fm_cand *out);

/* Reads to alignments: MEMs of every read (debwt_fm_mems, min_len, both strands unless DEBWT_FM_MAP_FORWARD), each MEM
 * located for at most max_occ rows (the first rows in suffix order), the seeds clustered per read
 * (debwt_fm_cluster_seeds with `band` and max_cand), one extension job per candidate, all jobs of a batch of reads in one
 * extension pass.  Per read the best score wins (ties by smaller (strand, record, tbeg)); sub = the best score of
 * another job of the read whose text interval does not intersect the winner's (0: none); mapq = 60 * (score - sub) /
 * score in integers.  A read without a seed or with a best score below min_score is unmapped (score 0,
 * DEBWT_FM_MAP_UNMAPPED); a read above 65535 bases is not extended (DEBWT_FM_MAP_UNMAPPED | DEBWT_FM_MAP_TOO_LONG).
 * A plain heuristic: neither the seeding strategy nor the mapping quality is BWA-MEM's.
 * hits[i]: read i.  qbeg .. tend, edits as debwt_fm_extend gives them (qbeg, qend in the read's reverse complement when
 * DEBWT_FM_MAP_REVERSE is set); offset = tbeg - first position of `record`; diag: the diagonal of the job that won, so a
 * caller can re-derive the band.  CIGARs through cigar_offsets (npat + 1) / cigar / capacity as in debwt_fm_extend
 * (DEBWT_ERANGE after hits and cigar_offsets are written). */
#define DEBWT_FM_MAP_REVERSE  1u   /* hit flag: aligned as the reverse complement */
#define DEBWT_FM_MAP_UNMAPPED 2u   /* hit flag */
#define DEBWT_FM_MAP_TOO_LONG 4u   /* hit flag */
#define DEBWT_FM_MAP_FORWARD  1u   /* option flag: seed and align the reads as given only */
typedef struct {
    uint32_t min_len;      /* shortest MEM used as a seed (19) */
    uint32_t band;         /* w of clustering and extension (16) */
    uint32_t max_occ;      /* rows located per MEM (64) */
    uint32_t max_cand;     /* candidates extended per read (8) */
    int32_t min_score;     /* below it a read is unmapped (30) */
    uint32_t flags;        /* DEBWT_FM_MAP_FORWARD */
    debwt_fm_scoring scoring;   /* (1, 4, 6, 1) */
} debwt_fm_map_opts;
typedef struct {
    uint64_t pattern;
    uint32_t flags, record;
    uint64_t offset;
    uint32_t qbeg, qend;
    uint64_t tbeg, tend;
    int32_t score, sub;
    uint32_t mapq, edits;
    int64_t diag;
} debwt_fm_hit;
void debwt_fm_map_defaults(debwt_fm_map_opts *opts);
/* opts NULL: the defaults */
int debwt_fm_map(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat, const debwt_fm_map_opts *opts,
                 debwt_fm_hit *hits, uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity);
/* the last debwt_fm_map: reads, reads mapped, seeds (located MEM occurrences), candidates kept (= extension jobs), and host
 * wall milliseconds per stage: MEMs, locate, candidate building, extension, and the whole call */
typedef struct {
    uint64_t reads, mapped, mems, seeds, candidates, jobs, batches;
    float ms_mems, ms_locate, ms_candidates, ms_extend, ms_wall;
} debwt_fm_map_stats;
int debwt_fm_map_stats_get(const debwt_fm *fm, debwt_fm_map_stats *out);

/* ---- chaining of seeds across diagonals, extension along a chain, and a mapper on both (fm_chain_kernels.h) ---------
 * Seeds of ONE read to colinear chains (host only, no GPU; the chaining step of debwt_fm_map_chained).
 * Seed quantities.  For seed x: len = qend - qbeg, tbeg = diag + qbeg, tend = diag + qend.  The seeds are sorted by
 * (strand, record, tbeg, qbeg, qend).  Indices below are positions in that order.
 * Valid predecessor.  i < j is a valid predecessor of j iff all of these hold: strand and record agree;
 * qbeg_i < qbeg_j, qend_i < qend_j, tbeg_i < tbeg_j, tend_i < tend_j; |diag_j - diag_i| <= band;
 * qbeg_j - qend_i <= max_gap and tbeg_j - tend_i <= max_gap, as signed values.  Overlaps are allowed.
 * Gain and DP.  gain(i,j) = min(len_j, qend_j - qend_i, tend_j - tend_i) - |diag_j - diag_i|;
 * f(j) = max(len_j, max over valid i of f(i) + gain(i,j)).
 * Predecessor tie rule.  The predecessor is the i that reaches the maximum.  Among several, the largest i wins.  "No
 * predecessor" is taken only when it is strictly better than every i.
 * Chain extraction.  Take the seeds in descending f, ties by smaller index.  A seed not yet used ends a chain.  Walk its
 * predecessors back until there is none, or until the next one is already used.  The used one is not part of the chain.
 * Mark the chain's seeds used.  score = f(end) - f(first used seed met), or f(end) when none was met.
 * Output.  The max_chains chains of the largest score are written, largest first, ties by smaller (strand, record, first
 * anchor's diag, first anchor's qbeg), then by the order of extraction.  A chain's anchors are its seeds in ascending
 * qbeg, as (qbeg, diag), at anchors[first_anchor .. first_anchor + n_anchors).  By the validity rule qbeg strictly
 * increases and consecutive diag differ by at most band.  The function returns the number of chains written.
 * *anchors_needed (the anchors of the chains written) is written first, then the chains; DEBWT_ERANGE when
 * anchor_capacity is smaller than *anchors_needed (no anchor is written then), following the protocol of
 * debwt_fm_locate.  DEBWT_EINVAL for a seed with qend <= qbeg, or for band > 63.
 * The sort order lets the inner loop stop early: going back from j, once tbeg_j - tbeg_i exceeds max_gap plus the longest
 * seed no earlier i can be valid.  No result depends on that. */
typedef struct {
    uint32_t qbeg;
    uint32_t reserved;
    int64_t diag;
} debwt_fm_anchor;
typedef struct {
    int32_t score;
    uint32_t record, strand, n_anchors;
    uint64_t first_anchor;
} debwt_fm_chain;
int debwt_fm_chain_seeds(const debwt_fm_seed *seeds, uint64_t nseeds, uint32_t band, uint32_t max_gap,
                         uint32_t max_chains, debwt_fm_chain *chains, debwt_fm_anchor *anchors,
                         uint64_t anchor_capacity, uint64_t *anchors_needed);

/* Banded affine-gap local alignment of jobs along chains.  Everything is as debwt_fm_extend documents it -- the
 * recurrence for E, F, H and the score, the scoring limits and Q, strand handling and out[], the CIGAR coding, the
 * DEBWT_ERANGE protocol and the score-only mode, the rule for the end cell and the traceback tie rule -- except the set
 * of allowed cells.  With the job's anchors (q_0, d_0) .. (q_{r-1}, d_{r-1}) = anchors[first_anchor .. first_anchor +
 * n_anchors), the band centre of query row i is c(i) = d_a for the largest a with q_a <= i, and c(i) = d_0 for i < q_0.
 * Cell (i, t) is allowed iff 0 <= i < m, rs <= t < re and |t - i - c(i)| <= w.  A job with one anchor is exactly a
 * debwt_fm_extend job with diag = d_0: the same out, the same CIGAR and the same offsets, bit for bit.  The total drift
 * d_{r-1} - d_0 is not limited.  The result does not depend on how the jobs are batched.
 * DEBWT_EINVAL in addition to the cases of debwt_fm_extend: n_anchors == 0, anchors out of range of the `anchors` array,
 * qbeg not strictly increasing or >= m, consecutive diagonals further apart than band.  DEBWT_ESTATE without an attached
 * text.  Device scratch: (rows that hold an allowed cell) x (2w + 1) flag bytes per job with a traceback; batches are cut
 * at DEBWT_FM_EXTEND_BYTES of it, as in debwt_fm_extend.  debwt_fm_extend_stats_get reports the last chain extension
 * too; its "wave steps" are then query rows (one row of 2w + 1 band indices each), not anti-diagonals. */
typedef struct {
    uint64_t pattern;
    uint32_t record, strand;
    uint64_t first_anchor;
    uint32_t n_anchors, reserved;
} debwt_fm_chain_job;
int debwt_fm_extend_chain(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                          const debwt_fm_chain_job *jobs, uint64_t njobs, const debwt_fm_anchor *anchors, uint64_t nanchors,
                          const debwt_fm_scoring *scoring, uint32_t band, debwt_fm_aln *out,
                          uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity);

/* Reads to alignments through chains: the stages of debwt_fm_map with debwt_fm_chain_seeds (band, max_gap, max_cand
 * chains kept) in place of debwt_fm_cluster_seeds and one debwt_fm_extend_chain job per chain, so a read whose indels
 * move it more than `band` diagonals away from a seed is still aligned end to end, as long as seeds on the way let the
 * band follow it in steps of at most `band`.  The winner, sub, mapq, the flags, the unmapped / too-long rules and the
 * DEBWT_ERANGE protocol are those of debwt_fm_map; hits[i].diag is the first anchor's diagonal of the winning chain.
 * anchor_offsets (npat + 1) and hit_anchors return the winning chain's anchors per read (none for an unmapped read), so
 * that a caller can rebuild the band; both may be NULL; DEBWT_ERANGE when anchor_capacity < anchor_offsets[npat], after
 * anchor_offsets is written.  debwt_fm_map_stats_get describes the last mapping call of either kind; ms_candidates then
 * holds the chaining time (host, at most 16 threads across reads) and candidates the chains kept.
 * max_gap: the longest stretch, in the read or in the text, between two consecutive seeds of a chain (5000). */
typedef struct {
    debwt_fm_map_opts map;
    uint32_t max_gap;
    uint32_t reserved;
} debwt_fm_chain_opts;
void debwt_fm_chain_defaults(debwt_fm_chain_opts *opts);
/* opts NULL: the defaults */
int debwt_fm_map_chained(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                         const debwt_fm_chain_opts *opts, debwt_fm_hit *hits,
                         uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity,
                         uint64_t *anchor_offsets, debwt_fm_anchor *hit_anchors, uint64_t anchor_capacity);

/* ---- paired-end reads: alignment against a text window, insert bounds, pair selection, the pair mapper
 * (fm_window_kernels.h) ----------------------------------------------------------------------------------------------
 * Affine-gap local alignment of jobs against text windows.  Everything is as debwt_fm_extend documents it -- Q and the
 * strand handling, the recurrence for E, F, H and the score, the scoring limits, out[] and the BAM-coded CIGAR, the
 * DEBWT_ERANGE protocol and the score-only mode with cigar_offsets NULL, the rule for the end cell (largest H, then the
 * smallest query index, then the smallest text position), the traceback tie rule and the independence from batching --
 * except the set of allowed cells.  With [rs, re) the bases of `record`, cell (i, t) is allowed iff 0 <= i < m and
 * max(rs, wbeg) <= t < min(re, wend), wbeg and wend being global text positions.  There is no band.  A window that misses
 * the record gives score 0 (empty CIGAR, coordinates 0); it is not an error.
 * DEBWT_EINVAL: m outside 1..DEBWT_FM_WINDOW_MAX_QUERY, wend < wbeg, wend - wbeg > DEBWT_FM_WINDOW_MAX_COLUMNS, pattern >=
 * npat, strand > 1, record >= nrec, a scoring value out of range.  DEBWT_ESTATE without an attached text.
 * Device scratch with a traceback: 64 flag bytes per step of the job's wave; a window of L columns has ceil(L / 64)
 * strips and a strip of c columns m + c - 1 steps, so a job takes at most 64 x ceil(L / 64) x (m + 63) bytes.  Batches
 * are cut at DEBWT_FM_EXTEND_BYTES of it, as in debwt_fm_extend; a job above that goes alone.
 * debwt_fm_extend_stats_get reports the last window pass too; a wave step is then one anti-diagonal of one strip of 64
 * columns, so cells / (64 x wave_steps) is the share of busy lanes. */
#define DEBWT_FM_WINDOW_MAX_QUERY   4096u    /* longest query of a window job */
#define DEBWT_FM_WINDOW_MAX_COLUMNS 16384u   /* widest window, wend - wbeg */
typedef struct {
    uint64_t pattern;
    uint32_t record, strand;
    uint64_t wbeg, wend;
} debwt_fm_window_job;
int debwt_fm_align_window(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                          const debwt_fm_window_job *jobs, uint64_t njobs, const debwt_fm_scoring *scoring,
                          debwt_fm_aln *out, uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity);

/* Insert-size bounds from observed template lengths (host only, no GPU).  On a sorted copy s of tlen[0 .. n):
 * q1 = s[n / 4], q3 = s[3 n / 4], d = q3 - q1; *lo = max(1, q1 - 3 d) in signed arithmetic, *hi = min(16384, q3 + 3 d).
 * DEBWT_EINVAL for n < DEBWT_FM_INSERT_MIN_PAIRS.  The quartile rule and the 32 are common practice, not measurements. */
#define DEBWT_FM_INSERT_MIN_PAIRS 32u
#define DEBWT_FM_INSERT_MAX       16384u
int debwt_fm_insert_bounds(const uint64_t *tlen, uint64_t n, uint32_t *lo, uint32_t *hi);

/* The choice of one pair from the candidate alignments of its two mates (host only, no GPU).  c1[0 .. n1), c2[0 .. n2):
 * score, record, strand and the global text interval [tbeg, tend) of each candidate; flags are not read.
 * Eligible.    A candidate is eligible when score >= max(1, min_score).
 * Single best. b(x) is mate x's eligible candidate of largest score, ties by smaller (strand, record, tbeg), then by
 *              smaller index; -1 when there is none.
 * Proper pair. (i, j) is a proper pair when both are eligible, the record is the same, the strands differ, and, with f
 *              the strand-0 one and r the strand-1 one, tbeg_f <= tbeg_r, tend_f <= tend_r and
 *              ins_lo <= T = tend_r - tbeg_f <= ins_hi.
 * Pair score.  P = score_i + score_j.  The best proper pair is the one with the largest P, ties by smaller
 *              (record, tbeg_f, i, j).
 * Choice.      The best proper pair is chosen iff one exists and P >= score(b1) + score(b2) - unpaired_penalty.  Then
 *              i1 = i, i2 = j, proper = 1, tlen = T and pair_score = P.
 * Otherwise.   i1 = b1, i2 = b2, proper = 0 and tlen = pair_score = pair_sub = 0.
 * pair_sub.    The largest P' of a proper pair (i', j') whose i' interval does not intersect the chosen i1's, or whose
 *              j' interval does not intersect the chosen i2's; 0 when there is none.
 * sub_x.       The largest score > 0 of another candidate of mate x, eligible or not, whose interval does not intersect
 *              the chosen one's (the rule of debwt_fm_map); 0 when there is none or mate x has no choice.
 * mapq_x.      single_x = 60 (s - sub_x) / s in integers, s the chosen score (0 without a choice).  For a proper pair
 *              mapq_x = max(single_x, 60 (P - pair_sub) / P).
 * DEBWT_EINVAL for ins_lo > ins_hi or a candidate with tend <= tbeg and score > 0. */
typedef struct {
    int32_t score;
    uint32_t record, strand, flags;
    uint64_t tbeg, tend;
} debwt_fm_pcand;
typedef struct {
    int32_t i1, i2;
    uint32_t proper, mapq1, mapq2;
    int32_t sub1, sub2, pair_score, pair_sub;
    int64_t tlen;
} debwt_fm_pair_choice;
int debwt_fm_pair_select(const debwt_fm_pcand *c1, uint32_t n1, const debwt_fm_pcand *c2, uint32_t n2,
                         uint32_t ins_lo, uint32_t ins_hi, int32_t unpaired_penalty, int32_t min_score,
                         debwt_fm_pair_choice *out);

/* Paired-end reads to alignments.  Patterns 2p and 2p + 1 are the mates of pair p; hits and cigar_offsets have 2 npairs
 * (+ 1) entries with the meanings debwt_fm_map gives them.  DEBWT_FM_MAP_FORWARD in map.flags is DEBWT_EINVAL.
 * 1. Candidates.  The stages MEMs, locate, cluster, extend of debwt_fm_map over all reads, keeping every job's alignment
 *    and CIGAR.  All batches finish before stage 2, so no result depends on the internal batching.
 * 2. Insert bounds.  With ins_lo = ins_hi = 0 they are estimated: the pairs whose two single bests have a single mapq >=
 *    20, share a record, have opposite strands and the forward-before-reverse geometry of debwt_fm_pair_select with
 *    T <= 16384 give their T, in pair order, to debwt_fm_insert_bounds.  Fewer than 32 such pairs: DEBWT_EINVAL, and
 *    debwt_fm_last_error asks for explicit bounds.
 * 3. Rescue (skipped for max_rescue = 0).  For each mate x and each of its max_rescue best eligible candidates c, in
 *    the single-best order: when the other mate y has no eligible candidate that forms a proper pair with c, and y has at
 *    most DEBWT_FM_WINDOW_MAX_QUERY bases, one window job aligns y on strand 1 - strand(c) in record(c), in the window
 *    [tbeg_c, tbeg_c + ins_hi) for strand(c) = 0, else [max(0, tend_c - ins_hi), tend_c).  Identical jobs are issued
 *    once; all jobs of the call go through debwt_fm_align_window with tracebacks.  A result with score >= min_score that
 *    is not identical (strand, tbeg, tend) to an existing candidate of y joins y's candidates, marked rescued.
 * 4. Selection.  debwt_fm_pair_select per pair; the hits are filled as debwt_fm_map fills them, sub and mapq being the
 *    choice's.  A rescued winner has diag = tbeg - qbeg and DEBWT_FM_MAP_RESCUED; DEBWT_FM_MAP_PROPER is set on both
 *    mates of a proper pair.  A mate without a choice is unmapped, under the rules of debwt_fm_map.
 * pairs[p]: tlen (T of a proper pair, else 0), pair_score and pair_sub of the choice. */
#define DEBWT_FM_MAP_PROPER  8u    /* hit flag */
#define DEBWT_FM_MAP_RESCUED 16u   /* hit flag */
typedef struct {
    debwt_fm_map_opts map;
    uint32_t ins_lo, ins_hi;      /* 0, 0: estimated from the reads */
    uint32_t max_rescue;          /* candidates of a mate that may start a rescue of its partner (4) */
    int32_t unpaired_penalty;     /* 17, BWA-MEM's */
} debwt_fm_pair_opts;
typedef struct {
    int64_t tlen;
    int32_t pair_score, pair_sub;
    uint32_t reserved;
} debwt_fm_pair_info;
void debwt_fm_pair_defaults(debwt_fm_pair_opts *o);
/* opts NULL: the defaults */
int debwt_fm_map_pairs(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npairs,
                       const debwt_fm_pair_opts *opts, debwt_fm_hit *hits, debwt_fm_pair_info *pairs,
                       uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity);
/* the last debwt_fm_map_pairs: pairs, proper pairs, window jobs of the rescue, rescued alignments that won, the insert
 * bounds used, the pairs the estimate used (0 with explicit bounds), and host wall milliseconds of the candidates,
 * the rescue, the selection and the whole call */
typedef struct {
    uint64_t pairs, proper, rescue_jobs, rescued, ins_lo, ins_hi, estimate_pairs;
    float ms_candidates, ms_rescue, ms_select, ms_wall;
} debwt_fm_pair_stats;
int debwt_fm_pair_stats_get(const debwt_fm *fm, debwt_fm_pair_stats *out);
/* ---- extract: record text and the whole text from the index alone (fm_extract_kernels.h) --------------------------
 * The third query of an FM-index.  Both calls below need the rows, the separator rows and the samples only: an index
 * from debwt_fm_open answers exactly as one from debwt_fm_create.
 * Anchors.  The first call of either kind orders the samples by text position on the device (8 bytes per sample: a
 * permutation of sample numbers; position and row follow from it) and keeps the list with the index: it is counted in
 * debwt_fm_info.device_bytes from then on, as the record table of debwt_fm_overlaps is.  It is built from a bitmap of
 * the sampled positions and a rank over it (n / 8 + n / 16 bytes while it is built, released afterwards), so it has no
 * capacity below the index's own.  The samples are checked on the way: every position < n, all distinct; otherwise
 * DEBWT_EINVAL with the reason in debwt_fm_last_error, and no anchors are kept.
 * Every walk takes a number of LF steps fixed by two checked positions: samples that are not the rows' can give wrong
 * letters or DEBWT_EINVAL, never an endless walk or a store outside the output.
 *
 * debwt_fm_extract.  Job j yields S_record[offset, min(offset + length, |S_record|)) as upper-case ACGT: length
 * UINT64_MAX means "to the end"; offset == |S_record| and length == 0 are legal and yield nothing.  DEBWT_EINVAL for
 * record >= nrec, offset > |S_record| or reserved != 0.  out_offsets (njobs + 1) are the prefix sums of the lengths and
 * are written first; DEBWT_ERANGE when capacity < out_offsets[njobs] (the protocol of debwt_fm_locate).  bases
 * [out_offsets[j], out_offsets[j + 1]) is job j's text; no terminator is written.  A walk that misses the row of its
 * anchor or meets a separator inside a record is DEBWT_EINVAL (the samples are not those of the rows).
 * Batches are cut inside the library at DEBWT_FM_EXTRACT_BYTES output bytes (environment, read per call; default 256 MiB)
 * and 2^22 jobs; a job above the limit goes alone.  A job is cut into one walk per gap between sampled positions, so a
 * long job is as parallel as many short ones.  The result depends on neither the limit nor on sa_sample.  Device
 * scratch: the bytes of one batch, 40 bytes per job of it, each with up to 25 % slack. */
typedef struct { uint32_t record, reserved; uint64_t offset, length; } debwt_fm_extract_job;
int debwt_fm_extract(debwt_fm *fm, const debwt_fm_extract_job *jobs, uint64_t njobs,
                     uint64_t *out_offsets, char *bases, uint64_t capacity);
/* what the last debwt_fm_extract or debwt_fm_restore_text did: jobs (0 for a restore), batches, kernel launches (plan and
 * walk per batch; walk, padding and text check for a restore), segments (walks between two anchors), bases (n for a
 * restore), LF steps (one v_lf each), wave steps (64 x the loop iterations per wave: steps / wave_steps is the share of
 * lanes busy), rank lines read, the bytes of the anchors, the time to build them (events; 0 when they existed), walk
 * time (events) and host wall time */
typedef struct {
    uint64_t jobs, batches, launches, segments, bases, steps, wave_steps, line_reads, anchor_bytes;
    float ms_anchors, ms_kernel, ms_wall;
} debwt_fm_extract_stats;
int debwt_fm_extract_stats_get(const debwt_fm *fm, debwt_fm_extract_stats *out);
/* debwt_fm_attach_text without a source: the 2-bit text is rebuilt in HBM from the index alone and attached.  DEBWT_OK at
 * once when a text is attached already.  Afterwards the text is counted in debwt_fm_info.device_bytes and every call
 * that wants a text works.  A text is attached only if every segment between two anchors arrives on the row of its
 * lower anchor (the chain condition of the verifier's walk), the first segment ends on the '$' symbol, the positions
 * at which '#' was met are exactly the record starts - 1 with '$' met nowhere but before position 0, and the check of
 * debwt_fm_attach_text finds nothing; otherwise DEBWT_EINVAL with the reason in debwt_fm_last_error, and no text is
 * attached.  debwt_fm_extract_stats_get describes it, with jobs = 0 and bases = n. */
int debwt_fm_restore_text(debwt_fm *fm);
/* The attached text to the host, however it was attached: packed receives ((n + 63) >> 5) + 2 words in the format
 * debwt_load_text takes (32 'T' behind position n - 1, zeros behind), sep the nrec separator positions -- enough to
 * load a context and build again with another k.  DEBWT_ESTATE without a text, DEBWT_ERANGE when capacity_words is
 * below the word count. */
int debwt_fm_text_fetch(debwt_fm *fm, uint64_t *packed, uint64_t capacity_words, uint64_t *sep);
/* ---- k-mer counts along reads and k-mer read correction (fm_kmer_kernels.h) ----------------------------------------
 * Characters: A/C/G/T in either case are bases, every other byte is a non-base.  For a string W of k bytes, occ W is 0
 * when W holds a non-base and otherwise what debwt_fm_count reports for it, hi - lo: the occurrences inside one record.
 * cnt W = occ W, and with DEBWT_FM_BOTH_STRANDS cnt W = occ W + occ revcomp W (A<->T, C<->G): a k-mer that equals its
 * own reverse complement is therefore counted TWICE.  None of the calls below needs an attached text: an index from
 * debwt_fm_open answers as one from debwt_fm_create.
 *
 * debwt_fm_kmer_counts.  Pattern i of m bytes has nk = max(0, m - k + 1) k-mers.  count_offsets (npat + 1) are the prefix
 * sums of nk and are written first; DEBWT_ERANGE when capacity < count_offsets[npat] (the protocol of debwt_fm_locate).
 * counts[count_offsets[i] + j] = min(cnt of P_i[j .. j + k), 2^32 - 1).  DEBWT_EINVAL for k = 0, flags other than
 * DEBWT_FM_BOTH_STRANDS, decreasing offsets and a pattern of 2^32 bytes or more.
 * Batches are cut inside the library at 64 MB of pattern bytes and DEBWT_FM_KMER_ITEMS k-mer positions (environment, read
 * per call; default 2^24; a pattern with more goes alone); the result depends on neither.  Device scratch of a batch, each
 * with up to 25 % slack: the pattern bytes, 16 bytes per pattern and 4 per position (64 MiB at the default); the
 * correction adds 13 bytes per position and 34 per pattern (about 300 MiB in all at the default).
 *
 * The prefix table.  For every q-mer w the table holds the [lo, hi) that debwt_fm_count gives for w: 2 u64 per entry,
 * 16 * 4^q bytes, the first character the most significant digit.  It is made on the device, level by level, by the
 * first call that needs it (q > 0 and k >= q; a call with k < q uses none and reports table_q 0), and kept with the index like the record table of debwt_fm_overlaps: from then on it is
 * counted in debwt_fm_info.device_bytes.  A k-mer with k >= q starts from the entry of its last q characters and walks
 * the remaining k - q; a k-mer with k < q walks from [0, n).  q is DEBWT_FM_KMER_TABLE_Q (environment, read per call;
 * 0..12, default 12: 268 MB; 0 = no table, anything else DEBWT_EINVAL); a kept table of another q is replaced.  No result
 * depends on q. */
int debwt_fm_kmer_counts(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat, uint32_t k,
                         uint32_t flags, uint64_t *count_offsets, uint32_t *counts, uint64_t capacity);
/* what the last debwt_fm_kmer_counts did (and, inside debwt_fm_correct_stats, the last debwt_fm_correct): patterns,
 * batches, kernel launches (the table's levels included), k-mers counted (positions; for a correction also the
 * substituted k-mers of the trials), rank steps (one fm_occ2 each), rank lines read, wave steps (64 x the longest lane
 * per wave: steps / wave_steps is the share of lanes busy, the rest idle behind k-mers that died), the walks started
 * from a table entry (per k-mer and strand), the largest scratch of a batch, the table's q (0: none used), the time to
 * build the table (events; 0 when it existed), kernel time (events) and host wall time */
typedef struct {
    uint64_t patterns, batches, launches, kmers, steps, line_reads, wave_steps, table_starts, scratch_bytes;
    uint32_t table_q, reserved;
    float ms_table, ms_kernel, ms_wall;
} debwt_fm_kmer_stats;
int debwt_fm_kmer_stats_get(const debwt_fm *fm, debwt_fm_kmer_stats *out);
/* Weak runs and trials of one read, on the host (no GPU).  counts are the nk counts of its k-mers.  k-mer j is weak iff
 * counts[j] < min_count; a run [a, b] is a maximal interval of weak k-mers, len = b - a + 1.  Each run yields up to two
 * trials (pos, window), the left one first:
 *   left  (kind 0) when a > 0 and (len >= k or b == nk - 1):       pos = a + k - 1, window = a;
 *   right (kind 1) when b < nk - 1 and (len >= k or a == 0):       pos = b,         window = b.
 * This is the signature of one substitution at pos: every k-mer over pos is weak, and window is the weak k-mer next to a
 * solid one.  A run that covers the whole read has no trial, and interior runs shorter than k are left alone.
 * Trials are written runs ascending; the call returns the number of trials of the read and writes the first `capacity`
 * of them (out may be NULL when capacity is 0), so a return above capacity names the capacity to come back with.
 * DEBWT_EINVAL for k = 0, min_count = 0 and nk + k above 2^31. */
typedef struct { uint32_t run_a, run_b, pos, window, kind; } debwt_fm_trial;
int debwt_fm_weak_trials(const uint32_t *counts, uint64_t nk, uint32_t k, uint32_t min_count, debwt_fm_trial *out,
                         uint64_t capacity);
/* Read correction from the k-mer spectrum of the indexed collection.  out has the layout of patterns and the same
 * offsets.  Per read R of m >= k bytes, at most max_rounds times:
 *   1. cnt of all nk k-mers of the current R; if none is weak (cnt < min_count), stop;
 *   2. the trials of debwt_fm_weak_trials; per run they are evaluated in order, left first;
 *   3. a trial (pos, window) tests every x of A, C, G, T other than upper R[pos] (all four when R[pos] is a non-base):
 *      W_x is R[window .. window + k) with position pos replaced by x, and x is a candidate iff cnt W_x >= min_count;
 *   4. the trial succeeds iff there is exactly one candidate; a run's fix is that of its first successful trial;
 *   5. if no run has a fix, stop; otherwise all fixes are applied, R[pos] := x in upper case.
 * The fixes of one round fall on distinct positions.  Bytes that are not fixed stay as given, case included.
 * info[i] = {flags, fixes, weak_before, weak_after}; weak_after is counted on the output read, and exactly one flag is
 * set: DEBWT_FM_CORRECT_SHORT (m < k: the read is copied, the other fields are 0), DEBWT_FM_CORRECT_CLEAN (weak_before ==
 * 0), DEBWT_FM_CORRECT_FIXED (weak_before > 0, weak_after == 0), DEBWT_FM_CORRECT_WEAK (weak_after > 0).
 * Every count, the resolution and the write into the read bytes run on the device; between rounds only the number of
 * reads that got a fix reaches the host.  Batches as debwt_fm_kmer_counts; the result depends on neither limit nor on q.
 * DEBWT_EINVAL for k = 0, min_count = 0, max_rounds outside 1..16, flags other than DEBWT_FM_BOTH_STRANDS, decreasing
 * offsets and a pattern of 2^31 bytes or more. */
#define DEBWT_FM_CORRECT_SHORT 1u
#define DEBWT_FM_CORRECT_CLEAN 2u
#define DEBWT_FM_CORRECT_FIXED 4u
#define DEBWT_FM_CORRECT_WEAK  8u
#define DEBWT_FM_CORRECT_MAX_ROUNDS 16
typedef struct { uint32_t k, min_count, max_rounds, flags; } debwt_fm_correct_opts;
typedef struct { uint32_t flags, fixes, weak_before, weak_after; } debwt_fm_correct_info;
/* min_count 3, max_rounds 4, both strands; k is set to 0: it has no default */
void debwt_fm_correct_defaults(debwt_fm_correct_opts *opts);
int debwt_fm_correct(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                     const debwt_fm_correct_opts *opts, char *out, debwt_fm_correct_info *info);
/* what the last debwt_fm_correct did: the counters above over all its kernels, the largest number of rounds a batch
 * ran, per round the reads that got a fix (they stay active) and the time of its kernels (events), trials evaluated,
 * fixes applied, and the reads per flag */
typedef struct {
    debwt_fm_kmer_stats kmers;
    uint64_t rounds, trials, fixes, reads_short, reads_clean, reads_fixed, reads_weak;
    uint64_t active[DEBWT_FM_CORRECT_MAX_ROUNDS];
    float ms_round[DEBWT_FM_CORRECT_MAX_ROUNDS];
} debwt_fm_correct_stats;
int debwt_fm_correct_stats_get(const debwt_fm *fm, debwt_fm_correct_stats *out);

/* ---- Definition 9 (spectrum): the k-mer spectrum of the indexed collection (fm_spectrum_kernels.h) -------------------
 * k is in 1..32.  A k-mer W is written as a u64 code: A, C, G, T = 0..3, the first character in the most significant
 * digit, value below 4^k; code order equals string order.  occ W is as in the k-mer section above: the occurrences inside
 * one record, what debwt_fm_count answers; a k-mer that would span a separator or the end does not exist.
 *   Forward.  D is the set of W with occ W > 0, mult W = occ W.
 *   DEBWT_FM_BOTH_STRANDS.  D is the set of canonical codes m = min(W, revcomp W) with occ m + occ revcomp m > 0, and
 *   mult m = cnt of the k-mer section = occ m + occ revcomp m.  A k-mer equal to its own reverse complement therefore has
 *   mult 2 occ, exactly the number debwt_fm_correct compares with min_count.
 * Histogram, nbins in 2..4096: hist[0] = 0; for 1 <= c < nbins - 1 hist[c] = the number of W in D with mult = c;
 * hist[nbins - 1] = the number with mult >= nbins - 1.  Totals: distinct = |D| = the sum of hist, total = the sum of
 * mult over D, overflow_total = the sum of mult over the members of the last bin.
 *   forward:       total = the sum over the records S of max(0, |S| - k + 1);
 *   both strands:  total = the forward total + the sum of occ over the k-mers that equal their own reverse complement
 *                  (not twice the forward total: W and revcomp W share one member).
 * List: the members of D with min_mult <= mult <= max_mult, ascending by code, mult clamped to u32 (2^32 - 1) before it
 * is compared and written.
 * Threshold (host, no GPU): valley = the smallest c in 1..nbins-3 with hist[c + 1] > hist[c]; peak = the c in
 * valley+1..nbins-2 with the largest hist[c], the smallest such c on ties; without such a c, valley = peak = 0 ("no
 * valley").  est_size = (total - the sum over c < valley of c * hist[c]) / peak, integer division, 0 when peak = 0.  The
 * min_count taken from a spectrum is valley: k-mers below it are weak.
 *
 * The walk.  A frontier entry is (lo, hi, code) of one string with a non-empty row interval.  The walk starts from the
 * non-empty entries of the prefix table of the k-mer section (same q, same DEBWT_FM_KMER_TABLE_Q, built by the first call
 * that needs it and counted in device_bytes) or, when k < q or q = 0, from [0, n); each level prepends A, C, G, T to every
 * entry with one read of its rank line(s), so every distinct k-mer is met once.  Both strands: a leaf looks up occ of its
 * reverse complement (k - q steps from the table) and emits the member when it holds the canonical code, or when its
 * reverse complement does not occur.  The start entries are cut, in table order, into chunks whose sum of hi - lo is at
 * most DEBWT_FM_SPECTRUM_ITEMS (environment, read per call; default 2^22; an entry above the limit goes alone); the
 * children of an interval are disjoint parts of it, so that sum bounds every frontier of the chunk.  Device scratch, each
 * buffer with up to 25 % slack: 48 bytes (60 for a list) per item of max(the limit, the largest start entry), 16 bytes per
 * 1024 table entries, and below 1 MiB of counters, histogram and list staging: about 200 MiB at the default (240 for a
 * list).  Without a table the one start entry is [0, n): 48 n bytes.  No result depends on the limit or on q.  Neither
 * call needs an attached text.  The list is sorted on the host. */
typedef struct { uint64_t distinct, total, overflow_total; } debwt_fm_spectrum_totals;
typedef struct { uint64_t valley, peak, est_size; } debwt_fm_spectrum_summary;
/* DEBWT_EINVAL for k outside 1..32, nbins outside 2..4096, flags other than DEBWT_FM_BOTH_STRANDS and NULL outputs */
int debwt_fm_spectrum(debwt_fm *fm, uint32_t k, uint32_t flags, uint32_t nbins, uint64_t *hist,
                      debwt_fm_spectrum_totals *totals);
/* count is written first; DEBWT_ERANGE when capacity < count (the protocol of debwt_fm_locate; capacity 0 with NULL
 * arrays is the sizing call).  DEBWT_EINVAL for k outside 1..32, unknown flags, min_mult = 0, min_mult > max_mult, a NULL
 * count and NULL arrays with capacity > 0. */
int debwt_fm_kmer_list(debwt_fm *fm, uint32_t k, uint32_t flags, uint32_t min_mult, uint32_t max_mult,
                       uint64_t *codes, uint32_t *mults, uint64_t capacity, uint64_t *count);
/* host only; DEBWT_EINVAL for NULL and nbins outside 2..4096 */
int debwt_fm_spectrum_threshold(const uint64_t *hist, uint32_t nbins, uint64_t total, debwt_fm_spectrum_summary *out);
/* what the last debwt_fm_spectrum or debwt_fm_kmer_list did: chunks, kernel launches (the table's levels and the sizing
 * pass included), levels walked per chunk (k - start depth), intervals expanded (one fm_occ4 each), leaves (intervals of
 * depth k), reverse-complement look-ups, rank steps (expansions plus the fm_occ2 of the look-ups), rank lines read, wave
 * steps (64 per wave of an expansion, 64 x the longest look-up of a wave: steps / wave_steps is the share of lanes
 * busy), the scratch of the call (sized by its largest chunk), the limit in force, the intervals of every depth
 * (level_intervals[d], d = start depth .. k), the table's q (0: none used), the time to build the table (events; 0 when
 * it existed), the time from the first chunk to the last kernel (events) and host wall time */
typedef struct {
    uint64_t chunks, launches, levels, expanded, leaves, lookups, steps, line_reads, wave_steps, scratch_bytes, items_limit;
    uint64_t level_intervals[33];
    uint32_t table_q, reserved;
    float ms_table, ms_kernel, ms_wall;
} debwt_fm_spectrum_stats;
int debwt_fm_spectrum_stats_get(const debwt_fm *fm, debwt_fm_spectrum_stats *out);

/* ---- Definition 10 (enhanced suffix array): suffix array, LCP array and record array (fm_esa_kernels.h) ---------------
 * The text T is r0 # r1 # ... $ with n symbols; the order is the index's: A < C < G < T < '#' < '$', all '#' equal,
 * suffixes compared symbol by symbol through separators.  Rows are the rows of the BWT, r = 0 .. n - 1.
 *   sa[r]   the text position of the suffix of row r, a u64: what debwt_fm_locate answers for that row.
 *   da[r]   the record j with start_j <= sa[r] <= start_j + |S_j|, a u32: the separator behind a record, and the '$',
 *           belong to that record.
 *   d(p)    the number of bases from p up to the next separator; 0 when T[p] is a separator.
 *   lcp[0]  = 0.  For r >= 1, lcp[r] is the largest h <= min(d(sa[r-1]), d(sa[r])) with T[sa[r-1] .. +h) = T[sa[r] .. +h):
 *           the common prefix of the two suffixes, cut at the first separator of either, so a row whose suffix starts
 *           with a separator has lcp 0.  Stored as u32: min(lcp, cap), cap = max_lcp, or 2^32 - 1 when max_lcp = 0.
 * Three facts the kernels rest on (tests/esa_ref.py asserts them):
 *   1. for rows a < b the cut common prefix of suffixes sa[a] and sa[b] is min(lcp[a+1 .. b]);
 *   2. with plcp[i] = lcp[row of position i], plcp[i+1] >= plcp[i] - 1 (Kasai's carry), for the capped values too;
 *   3. the number of distinct strings of k bases inside records is #{ r : lcp[r] < k <= d(sa[r]) }, exact for k <= cap.
 * Summary: max = the largest stored value, max_row = the first row that holds it, sum = the sum of the stored values,
 * capped = the rows whose stored value equals a non-zero max_lcp (0 when max_lcp = 0), pos_prev = sa[max_row - 1] and
 * pos = sa[max_row], the two places of the longest repeat (both sa[0] when max_row = 0: every value is 0), cap = the cap
 * in force.  Profile: distinct[k - 1] for k = 1 .. kmax is fact 3; kmax <= cap and kmax <= 4096.
 *
 * The build.  The text is restored first when none is attached (debwt_fm_restore_text).  The suffix array is written by
 * one walk over the gaps between the anchors of the extract section, every row once, under the chain check of that walk:
 * samples that are not the rows' give DEBWT_EINVAL and nothing is kept.  phi[sa[r]] = sa[r-1] is scattered, the text
 * positions are cut into chunks of DEBWT_FM_ESA_CHUNK positions (environment, read per call; default 256) and one lane
 * per chunk compares word-wise, 32 bases a step, carrying the match length minus one from a position to the next inside
 * its chunk: the work is at most n + chunks x cap symbols plus two words per position, not the sum of the LCP values.  No
 * result depends on the chunk length.  Device memory while building, beside the text ((n + 63) / 32 + 2 words) and the
 * anchors: 8 n (sa) + 8 n (phi) + 4 n (plcp) + 4 n (lcp) + 4 n (da, when kept) + 3 n / 16 (separator bitmap and its rank) +
 * 8 nrec + 33 KiB; kept afterwards, allocated exactly and counted in debwt_fm_info.device_bytes until released: 4 n (lcp), 8 n
 * (sa) with DEBWT_FM_ESA_SA, 4 n (da) with DEBWT_FM_ESA_DA.  When an allocation fails the call answers DEBWT_ENOMEM and
 * keeps nothing.  A second build replaces the first (which is released before the new one is made). */
#define DEBWT_FM_ESA_SA 1u
#define DEBWT_FM_ESA_DA 2u
#define DEBWT_FM_ESA_LCP_ARRAY 0
#define DEBWT_FM_ESA_SA_ARRAY  1
#define DEBWT_FM_ESA_DA_ARRAY  2
#define DEBWT_FM_ESA_MAX_K 4096u
/* DEBWT_EINVAL for flags other than the two above, and for DEBWT_FM_ESA_DA on an index of 2^32 records or more */
int debwt_fm_esa_build(debwt_fm *fm, uint32_t max_lcp, uint32_t flags);
/* rows [row_lo, row_lo + count) of one array to the host: which = DEBWT_FM_ESA_LCP_ARRAY (u32), _SA_ARRAY (u64) or
 * _DA_ARRAY (u32).  DEBWT_ESTATE without a build or for an array that was not kept, DEBWT_EINVAL for another `which`,
 * row_lo + count > n, or a NULL dst with count > 0. */
int debwt_fm_esa_fetch(debwt_fm *fm, int which, uint64_t row_lo, uint64_t count, void *dst);
typedef struct { uint64_t n, max, max_row, sum, capped, pos_prev, pos, cap; } debwt_fm_esa_summary;
/* DEBWT_ESTATE without a build */
int debwt_fm_esa_summary_get(const debwt_fm *fm, debwt_fm_esa_summary *out);
/* distinct receives kmax values (host; the difference array was reduced by the build).  DEBWT_ESTATE without a build,
 * DEBWT_EINVAL for kmax = 0, kmax > cap and kmax > 4096. */
int debwt_fm_esa_profile(debwt_fm *fm, uint32_t kmax, uint64_t *distinct);
/* releases the kept arrays; DEBWT_OK without a build too */
int debwt_fm_esa_release(debwt_fm *fm);
/* what the last debwt_fm_esa_build did: walk items (anchor gaps), LF steps (n - 1) and wave steps of the walk (64 x the
 * loop iterations per wave), chunks and the chunk length in force, symbols_compared (the symbol pairs the PLCP kernel
 * examined, a whole word step counting 32), plcp_wave_steps (64 x the word steps of the longest lane of every wave:
 * symbols_compared / 32 / plcp_wave_steps is the share of lanes busy), the device bytes allocated by the build and those
 * kept, ms per phase (events: walk, scatter, PLCP, rows with the reductions), the wall time of a text restore (0 when
 * a text was attached) and host wall time */
typedef struct {
    uint64_t walk_items, walk_steps, walk_wave_steps, chunks, chunk_len, symbols_compared, plcp_wave_steps, build_bytes,
        kept_bytes;
    float ms_walk, ms_scatter, ms_plcp, ms_rows, ms_text, ms_wall;
} debwt_fm_esa_stats;
int debwt_fm_esa_stats_get(const debwt_fm *fm, debwt_fm_esa_stats *out);

/* ---- Definition 11 (repeats): maximal and supermaximal repeats from the kept LCP array (fm_repeat_kernels.h) -----------
 * Rows, sa, lcp, d() and the symbol order are those of Definition 10.  L[r] is the BWT symbol of row r, the symbol in
 * front of sa[r]: A, C, G, T, '#' or '$' ('$' on the row with sa[r] = 0).
 *   Interval.  A triple (l, i, j) with l >= 1, i < j, lcp[i] < l, (j = n - 1 or lcp[j + 1] < l) and min(lcp[i+1 .. j]) = l.
 *     Its string w = T[sa[i] .. +l) holds bases only (lcp is cut at separators) and occurs j - i + 1 times inside records,
 *     at sa[i .. j].  Its representative row is the smallest r in (i, j] with lcp[r] = l: every interval has exactly one,
 *     and a row represents at most one interval.
 *   Left counts.  left[c], c = 0..3: the rows of [i, j] whose L is base c; left[4]: those whose L is '#' or '$' (the
 *     occurrence starts a record).  The five sum to j - i + 1.
 *   Maximal repeat.  An interval with max(left[0..3]) < j - i + 1: occurrences that start a record count as pairwise
 *     different on the left.
 *   Supermaximal repeat.  An interval with every lcp[i+1 .. j] == l and every left[0..3] <= 1.  It is maximal.
 *   Capped build (max_lcp = c != 0).  The intervals with l < c are exactly those of the uncapped array (capping keeps
 *     values below c, and keeps values above l above l).  The intervals of stored value c are not reported; the statistics
 *     count them as capped_intervals, whatever min_len is.
 * The list: the intervals with len >= min_len, min_occ <= count (<= max_occ when max_occ != 0) and of the kind asked for,
 * ascending by representative row.  A record names the interval by row_lo = i and count = j - i + 1; len = l; flags tells
 * whether it is maximal and supermaximal, for every kind.  The occurrences are debwt_fm_esa_fetch(SA, row_lo, count) when
 * the build kept sa; the call itself needs the LCP array alone and changes none of the kept arrays.
 *
 * The method.  A min/max hierarchy over lcp with fanout F (environment DEBWT_FM_REPEAT_FANOUT, read per call, a power of
 * two in 2..64, default 64; DEBWT_EINVAL otherwise; no result depends on it): level 0 is lcp, entry b of level t + 1 holds
 * min and max of entries [b F, (b + 1) F) of level t, n_0 = n and n_{t+1} = ceil(n_t / F) up to one entry: `levels` levels
 * of tree_bytes = 8 (n_1 + .. + n_levels) bytes, below 8 n / (F - 1) + 8 levels.  One lane per row r with l = lcp[r] >=
 * min_len searches the nearest p < r with lcp[p] <= l (r is a representative iff lcp[p] < l, and then i = p), the nearest
 * q > r with lcp[q] < l (j = q - 1, q = n without one) and the nearest q' > r with lcp[q'] > l; the values of (i, r) are
 * above l, so the interval is flat iff r = i + 1 and q' >= q (the third search runs only for r = i + 1 with every left[0..3]
 * <= 1, where it decides).  Every search ascends while a node cannot hold a hit and
 * descends into the first that can: at most 2 F entries per level, never a number that grows with the distance.  The left
 * counts are two rank lines per base.  Order comes from the device: a wave's reported rows are a ballot, the rank over those
 * masks is a row's place in the list.  Scratch, all released before the call returns: the tree, 1 KiB of counters and 16
 * bytes per workgroup (at most 4096); a call with capacity > 0 adds 16 n + 28 ceil(n / 64) + 8 (ceil(n / 16384) + 1) bytes
 * and 64 bytes per record.  A failed allocation is DEBWT_ENOMEM and leaves the kept arrays as they were. */
#define DEBWT_FM_REPEAT_MAXIMAL       0u   /* kind */
#define DEBWT_FM_REPEAT_SUPERMAXIMAL  1u
#define DEBWT_FM_REPEAT_INTERVALS     2u   /* every interval, left-diverse or not */
#define DEBWT_FM_REPEAT_IS_MAXIMAL      1u /* flags of a record */
#define DEBWT_FM_REPEAT_IS_SUPERMAXIMAL 2u
typedef struct { uint32_t min_len, kind; uint64_t min_occ, max_occ; } debwt_fm_repeat_opts;  /* max_occ 0 = no bound */
typedef struct { uint64_t row_lo, count, left[5]; uint32_t len, flags; } debwt_fm_repeat;      /* 64 bytes */
/* count is written first; DEBWT_ERANGE when capacity < count (the protocol of debwt_fm_kmer_list; capacity 0 with a NULL
 * out is the sizing call).  DEBWT_ESTATE without a build or after debwt_fm_esa_release.  DEBWT_EINVAL for a NULL opts or
 * count, min_len = 0, min_occ < 2, max_occ != 0 && max_occ < min_occ, an unknown kind, a NULL out with capacity > 0 and a
 * fanout that is no power of two in 2..64. */
int debwt_fm_repeats(debwt_fm *fm, const debwt_fm_repeat_opts *opts, debwt_fm_repeat *out, uint64_t capacity, uint64_t *count);
/* what the last debwt_fm_repeats did: rows (n), rows searched (stored value >= min_len, capped rows included),
 * representatives among them, intervals (representatives below the cap: len >= min_len, any count and kind), the maximal
 * and the supermaximal of those, capped_intervals (representatives whose stored value is the cap), reported, the longest
 * reported length and its row_lo (the lowest on ties; 0, 0 without a record), levels and the fanout in force, tree_bytes,
 * scratch_bytes (everything the call allocated, the tree included), search_steps (hierarchy nodes and level-0 entries read by
 * the three searches), wave_steps (64 x the reads of the longest lane of every wave: search_steps / wave_steps is the share
 * of lanes busy), rank_lines (rank lines read for left counts, the write pass included), ms per phase (events: tree, search,
 * write with its rank) and host wall time */
typedef struct {
    uint64_t rows, searched, representatives, intervals, maximal, supermaximal, capped_intervals, reported, longest_len,
        longest_row_lo, levels, fanout, tree_bytes, scratch_bytes, search_steps, wave_steps, rank_lines;
    float ms_tree, ms_search, ms_write, ms_wall;
} debwt_fm_repeat_stats;
int debwt_fm_repeat_stats_get(const debwt_fm *fm, debwt_fm_repeat_stats *out);

/* ---- Definition 12 (records): distinct records per LCP interval, multi-MUMs (fm_record_kernels.h) ---------------------
 * Rows, sa, da, lcp (the STORED array, capped or not) and intervals are those of Definitions 10 and 11.
 *   prev[r]  the largest r' < r with da[r'] = da[r], or none.
 *   dup      For every row r that has a prev, m(r) is the smallest row of (prev[r], r] that holds min(lcp[prev[r]+1 .. r]):
 *            the leftmost argmin.  dup[m] is the number of rows r with m(r) = m.  The sum of dup is n minus the number of
 *            records present in da.  P[r] = dup[0] + .. + dup[r].
 *   Closed range.  Rows [lo, hi) are closed when hi - lo <= 1, or every value of lcp[lo+1 .. hi-1] is above lcp[lo], and
 *            above lcp[hi] when hi < n.  Every interval (l, i, j) is the closed range [i, j + 1); so is the range
 *            debwt_fm_count answers for a pattern of bases whose length is at most the cap of the build.
 *   records(lo, hi)  0 for an empty range, else (hi - lo) - (P[hi-1] - P[lo]).
 *   Fact 4 (tests/record_ref.py asserts it).  For a closed range records(lo, hi) is the number of distinct values of
 *            da[lo .. hi).  A row r of the range with prev[r] >= lo is exactly a repeated record, and its m(r) lies in
 *            (lo, hi).  Conversely, were m(r) in (lo, hi) with prev[r] < lo, then lo lies in (prev[r], r] and lcp[lo] >=
 *            lcp[m(r)], but lcp[m(r)] is above lcp[lo]; r >= hi is ruled out the same way through lcp[hi].
 *   Not closed.  For such a range the value is still the formula's, in u64 arithmetic (it may wrap below 0), and the
 *            leftmost argmin makes it the same in every run, but it is NOT a record count.
 *   multi-MUM.  A maximal interval (Definition 11) with count = records = the number of records of the index: its string
 *            occurs exactly once in every record and can be extended on neither side.  With a bound q: count = records >= q.
 *
 * The build needs da (DEBWT_FM_ESA_DA) and lcp.  Keys da[r] << rb | r (rb the bits of n - 1) are sorted by the stable
 * radix passes over the db bits of nrec - 1 (ceil(db / 8) passes; rb + db > 64 is DEBWT_EINVAL): neighbours with equal da
 * are the pairs (prev[r], r).  One lane per pair finds the leftmost argmin on the min/max hierarchy of Definition 11 (same
 * fanout, same DEBWT_FM_REPEAT_FANOUT; no result depends on it) -- an ascent from both ends of at most 2 (F - 1) entries
 * per level and a descent of at most F per level, never a number that grows with r - prev[r] -- and adds 1 to dup[m] with
 * an integer atomic, whose sum does not depend on the order of arrival.  dup is u32 for n < 2^32 and u64 above.  A prefix
 * sum makes P, kept as plain u64: kept_bytes = 8 n, allocated exactly, counted in debwt_fm_info.device_bytes, released by
 * debwt_fm_esa_release, by the next debwt_fm_esa_build and by debwt_fm_destroy.  Peak of the build beside the kept arrays:
 * 16 n (keys and sort scratch) + 4 n (dup; 8 n above 2^32 rows) + the tree (below 8 n / (F - 1) + 8 levels) + 16 MiB
 * (radix workspace) + n / 32 (tile sums) + 8 n (P); everything but P is freed before the call returns.  DEBWT_ENOMEM keeps
 * nothing new and leaves the kept arrays, an earlier P included, as they were; a second successful call replaces the
 * first.  DEBWT_ESTATE without a build or without a kept da. */
int debwt_fm_records_build(debwt_fm *fm);
/* P[row_lo .. row_lo + count) to the host as u64.  DEBWT_ESTATE without debwt_fm_records_build, DEBWT_EINVAL for
 * row_lo + count > n or a NULL P with count > 0. */
int debwt_fm_records_fetch(debwt_fm *fm, uint64_t row_lo, uint64_t count, uint64_t *P);
/* records[k] = records(ranges[2k], ranges[2k + 1]), ranges as debwt_fm_count writes them.  DEBWT_EINVAL for hi > n or
 * lo > hi in any range (nothing is written then), DEBWT_ESTATE without debwt_fm_records_build. */
int debwt_fm_record_counts(debwt_fm *fm, const uint64_t *ranges, uint64_t nranges, uint64_t *records);
#define DEBWT_FM_RECORDS_UNIQUE 1u         /* flags of a filter: count == records, no record holds the string twice */
typedef struct { uint64_t min_records, max_records; uint32_t flags, reserved; } debwt_fm_record_filter;  /* max_records 0 = no bound */
/* debwt_fm_repeats with a filter on the records of every interval: the list holds the intervals that debwt_fm_repeats
 * lists for opts and whose records lie in [min_records, max_records] (and equal count with DEBWT_FM_RECORDS_UNIQUE), in
 * the same order; records[k] (capacity entries, may be NULL) is the records of out[k].  Protocol and error codes are
 * those of debwt_fm_repeats; DEBWT_EINVAL also for a NULL filter, min_records = 0, max_records != 0 && max_records <
 * min_records, unknown flags and a non-zero reserved; DEBWT_ESTATE also without debwt_fm_records_build.  With the filter
 * {1, 0, 0} the list equals that of debwt_fm_repeats byte for byte.  A lane of the search that has i and j reads P[j] and
 * P[i] and applies the filter before the row is reported; the write pass reads the two again for records[] (4 bytes of
 * scratch more per listed record, nothing per row).
 * debwt_fm_repeat_stats_get describes this call too (its counters before `reported` do not depend on the filter). */
int debwt_fm_repeats_records(debwt_fm *fm, const debwt_fm_repeat_opts *opts, const debwt_fm_record_filter *filter,
                             debwt_fm_repeat *out, uint32_t *records, uint64_t capacity, uint64_t *count);
/* what the last debwt_fm_records_build did: rows (n), pairs (rows with a prev), records_present (n - pairs: the distinct
 * values of da), sort_passes, levels and the fanout in force, rmq_steps (hierarchy nodes and level-0 entries read by the
 * range minima), wave_steps (64 x the reads of the longest lane of every wave: rmq_steps / wave_steps is the share of
 * lanes busy), build_bytes (everything the call allocated, P included), kept_bytes, ms per phase (events: keys and sort,
 * tree, pairs, scan) and host wall time */
typedef struct {
    uint64_t rows, pairs, records_present, sort_passes, levels, fanout, rmq_steps, wave_steps, build_bytes, kept_bytes;
    float ms_sort, ms_tree, ms_pairs, ms_scan, ms_wall;
} debwt_fm_records_stats;
int debwt_fm_records_stats_get(const debwt_fm *fm, debwt_fm_records_stats *out);

/* ---- Definition 13 (compacted de Bruijn graph): unitigs and edges of the k-mers of the collection (fm_cdbg_kernels.h) --
 * Rows, sa, da, lcp (the STORED array), d(), L[r] and the symbol order are those of Definitions 10 and 11.  k >= 1.
 * Forward strand only: a k-mer and its reverse complement are two nodes, and nothing joins them; the bidirected unitigs
 * over canonical k-mers are Definition 14, debwt_fm_cdbg_both, below.
 *   Node.  A string W of k bases with occ W > 0 inside records: Definition 9, forward, for any k.  Its interval is [i, e)
 *     with lcp[i] < k <= d(sa[i]) and e the next row with lcp < k, or n; occ W = e - i.  A row with d(sa[r]) < k always has
 *     lcp[r] < k: it starts a piece that is no node.
 *   Edge string.  A string of k + 1 bases with occ > 0 inside records; it runs from its first k bases to its last k.
 *     out(W) is the number of rows r of [i, e) with (r = i or lcp[r] = k) and d(sa[r]) >= k + 1.  in(W) is the number of
 *     bases c with a row of [i, e) whose L is c (an occurrence that starts a record adds nothing); the node that enters W
 *     by c holds row C[c] + occ(c, i).
 *   Link.  u -> v iff out(u) = 1, v is u's only successor, in(v) = 1 and u != v (the rule of Definition 4).
 *   Unitig.  A maximal chain of links; every node is in exactly one.  A node with no incoming link starts one.  A
 *     component in which every node has an incoming link is a cycle: it starts at its node of the lowest row and is flagged
 *     DEBWT_FM_CDBG_CIRCULAR, and the link into that node counts as an edge, not as a member link.  Unitigs are numbered by
 *     ascending row of their first node, the string order of their first k-mers.  The string is the first node's k bases
 *     and the last base of every later node, nodes + k - 1 bases; kmer_count is the sum of occ over the nodes.
 *   Edge.  Every edge string that is no member link runs from the LAST node of a unitig to the FIRST node of one (the
 *     same one, perhaps).  The list holds (from, to) in unitig numbers, ascending by (from, to); no pair occurs twice.
 * Three facts (tests/cdbg_ref.py asserts them), distinct[] as debwt_fm_esa_profile answers:
 *   1. the sum of nodes over the unitigs = distinct[k - 1];
 *   2. the sum of (nodes - 1) over the unitigs + the number of edges = distinct[k], the distinct (k+1)-mers;
 *   3. the sum of kmer_count = the sum over the records S of max(0, |S| - k + 1).
 * A record: row_lo = the first row of the first node's interval; seq_offset = where the unitig's string begins in seq,
 * ASCII A, C, G, T, the strings packed in unitig order (seq_bytes = the sum of nodes + k - 1).
 *
 * The method.  Needs a build with DEBWT_FM_ESA_SA and DEBWT_FM_ESA_DA whose cap is 0 or at least k + 1 (the call must tell
 * lcp = k from lcp > k), and the text (restored when none is attached); it changes none of the kept arrays.  Limit: an
 * index of fewer than 2^32 rows.  One lane per row writes a start bit (lcp < k), a node bit and an out bit; a rank over the
 * start bits numbers the pieces, out() is a difference of ranks over the out bits, in() and the predecessor come from
 * the rank line(s) of the two ends of the interval.  The chains are ranked by pointer doubling towards the first node over
 * a compacted list of the unfinished nodes, states in two buffers so that no lane reads what another writes in the round; a
 * cycle shows when the span of its lowest node comes back to it, with its length, so an input without cycles ends when
 * its longest chain is ranked, and one with cycles ranks them in a second phase after the cut: at most ceil(log2(longest))
 * + 1 rounds a phase.  Unitig numbers are the rank over a bitmap of first nodes; kmer_count is summed inside a wave before
 * one lane adds to the unitig (integer adds); the edge keys are ordered by the stable radix passes of
 * debwt_fm_records_build.  No result depends on launch geometry or on the order in which atomics arrive.
 * Scratch, all released before the call returns, pieces = the rows with lcp < k, nodes <= pieces: n / 2 bytes (three
 * bitmaps over the rows, the ranks of two), 8 nrec (separators), 45 bytes per piece (lo, out, link, successor mark, two
 * states of 16 bytes) + 3 pieces / 16 (first nodes and their rank) + 8 bytes per node (two lists); a call that writes
 * adds 48 bytes per unitig + 8 per 256 unitigs, seq_bytes, and 24 bytes per edge + 16 MiB (keys, sort scratch, the list;
 * radix workspace).  A failed allocation is DEBWT_ENOMEM and leaves the kept arrays as they were. */
#define DEBWT_FM_CDBG_CIRCULAR 1u
typedef struct { uint64_t row_lo, seq_offset, kmer_count; uint32_t nodes, flags; } debwt_fm_unitig;   /* 32 bytes */
typedef struct { uint32_t from, to; } debwt_fm_cdbg_edge;
typedef struct { uint64_t unitigs, seq_bytes, edges; } debwt_fm_cdbg_sizes;
/* sizes is written first; DEBWT_ERANGE when any capacity is below its size (the protocol of debwt_fm_repeats; all
 * capacities 0 with NULL arrays is the sizing call, which skips the write pass).  flags: none defined, must be 0.  An index
 * whose records are all shorter than k answers DEBWT_OK with all sizes 0.  DEBWT_EINVAL for k = 0, unknown flags, a NULL
 * sizes, a NULL array with capacity > 0, k + 1 above the cap of a capped build and an index of 2^32 rows or more;
 * DEBWT_ESTATE without a build or with a build that kept no sa or no da. */
int debwt_fm_cdbg(debwt_fm *fm, uint32_t k, uint32_t flags, debwt_fm_unitig *unitigs, uint64_t unitig_capacity,
                  uint8_t *seq, uint64_t seq_capacity, debwt_fm_cdbg_edge *edges, uint64_t edge_capacity,
                  debwt_fm_cdbg_sizes *sizes);
/* what the last debwt_fm_cdbg did: nodes, edge strings (the sum of out()), unitigs, the circular ones, links (member
 * links: edge_strings = links + edges), edges, the nodes of the longest unitig, seq_bytes, jump_rounds (rounds of both
 * ranking phases), jump_steps (node visits of those rounds), jump_wave_steps (64 x the waves the rounds launched:
 * jump_steps / jump_wave_steps is the share of lanes busy), rank_lines (rank lines read for left counts, the edges of a
 * write pass included), scratch_bytes (everything the call allocated), ms per phase (events: nodes = bits, ranks and lo;
 * links = degrees and links; rank = the rounds; write = unitigs, strings and edges) and host wall time */
typedef struct {
    uint64_t nodes, edge_strings, unitigs, circular, links, edges, longest_nodes, seq_bytes, jump_rounds, jump_steps,
        jump_wave_steps, rank_lines, scratch_bytes;
    float ms_nodes, ms_links, ms_rank, ms_write, ms_wall;
} debwt_fm_cdbg_stats;
int debwt_fm_cdbg_stats_get(const debwt_fm *fm, debwt_fm_cdbg_stats *out);

/* ---- Definition 14 (compacted de Bruijn graph over both strands): bidirected unitigs over canonical k-mers
 * (fm_bicdbg_kernels.h) ------------------------------------------------------------------------------------------------
 * Let D = (S_0, rc S_0, S_1, rc S_1, ...) be the doubled collection.  D is never built: rows, intervals and occ are those of
 * the index of S.  k must be odd, so that no k-mer is its own reverse complement.
 *   Oriented node.  A string W of k bases such that W or rc W occurs inside a record of S (a node of Definition 13).
 *     mirror(W) = rc W.  W is present when it occurs itself, and mated when rc W occurs too.
 *   Oriented edge string.  A string E of k + 1 bases such that E or rc E occurs inside a record; it runs from its first k
 *     bases to its last k.  out2(W) and in2(W) count the distinct oriented edge strings that leave and enter W: the
 *     successors of W are the right extensions of W in S and the complemented left extensions of rc W in S, the
 *     predecessors symmetrically, so in2(W) = out2(rc W).
 *   Link.  u -> w iff out2(u) = 1, w is u's only successor, in2(w) = 1, w != u and w != mirror(u).  The last clause refuses
 *     a hairpin: an edge string that is its own reverse complement joins a node to its own mirror.  `hairpins` counts the
 *     edge strings that this clause alone keeps from being links.  Links are closed under u -> w |-> mirror(w) -> mirror(u),
 *     and no maximal chain or cycle of links holds a node together with its mirror: oriented unitigs come in mirror
 *     pairs U, U'.
 *   Reported orientation.  Let w* be the k-mer of the lowest row among the members of U and U' that occur in S; there is
 *     one, and it lies in exactly one of the two.  The orientation that holds w* is reported, pairs are numbered by
 *     ascending row of w*, and row_lo is the first row of w*'s interval: strictly ascending.  (w* need not be the first
 *     node of a linear unitig.)
 *   Cycle.  A component in which every oriented node has an incoming link.  The reported one starts at w* and is flagged
 *     DEBWT_FM_CDBG_CIRCULAR; the link into its first node counts as an edge, and so does the mirror of that link.
 *   Record.  debwt_fm_unitig as it is.  nodes: the canonical k-mers of the chain; kmer_count: the sum over them of
 *     occ W + occ rc W in S; the string is the first node's k bases and the last base of every later node in the reported
 *     orientation, a member that does not occur in S spelled as the reverse complement of its mirror's occurrence;
 *     seq_offset and seq_bytes as in Definition 13.
 *   Edge.  from = 2a + oa, to = 2b + ob: unitig a is traversed as reported when o = 0 and reverse-complemented when o = 1.
 *     Every oriented edge string that is no member link runs from the last node of an oriented unitig to the first node of
 *     one.  The list holds every such pair once, ascending by (from, to), and is closed under (x, y) |-> (y ^ 1, x ^ 1); an
 *     edge string and its reverse complement that both occur in S give one pair.  A refused hairpin at the end of unitig a
 *     is the pair (2a, 2a + 1), its own mirror image.
 * Facts (tests/bicdbg_ref.py asserts them):
 *   1. the sum of nodes = the distinct canonical k-mers; for k <= 32, debwt_fm_spectrum(k, DEBWT_FM_BOTH_STRANDS).distinct;
 *   2. 2 x the sum of (nodes - 1) + the number of edges = the number of oriented edge strings;
 *   3. the sum of kmer_count = the sum over the records S of max(0, |S| - k + 1);
 *   4. where hairpins = 0 the answer is Definition 13 applied to D with each mirror pair folded into one record.
 *
 * The method.  Preconditions as debwt_fm_cdbg: a build with DEBWT_FM_ESA_SA and DEBWT_FM_ESA_DA whose cap is 0 or at least
 * k + 1, and the text (restored when none is attached); none of the kept arrays changes.  Limit: an index of fewer than
 * 2^31 rows, since an oriented id needs one bit more than a piece.  Row bits, piece ranks and lo[] are those of Definition
 * 13.  A present node v has oriented id v, the mirror of an unmated v has id pieces + v, the mirror of a mated v is
 * mate[v].  Mates: one lane per present node searches its reverse complement backward, reading itself forward from the
 * text and stepping with the complement, k rank steps.  Degrees: every forward edge string is met once from its target
 * and ORs itself and its mirror into two 4-bit masks per oriented id (successor bases, predecessor bases), the single
 * predecessor id beside them.  Links: one lane per oriented id; then the ranking rounds of Definition 13 unchanged over
 * the 2 x pieces ids.  Pairs: the lowest id of a chain by an atomic minimum aggregated inside a wave; a chain is reported
 * iff its minimum is below that of the chain of its first node's mirror; the unitig number is the rank over a bitmap with
 * one bit at each w*.  The unreported chain of a pair is never walked: its ends, and for a cycle the place of its cut,
 * are read from the reported one through the mirror.  Edges: every forward edge string and its mirror that are no member
 * links go out as keys, ordered by the stable radix passes, and equal neighbours are dropped by a rank over the bitmap of
 * the keys that differ from the one before; the number of edges is known before, oriented edge strings - 2 links.  No
 * result depends on launch geometry or on the order in which atomics arrive (OR, minimum and integer adds).
 * Scratch, all released before the call returns: 3 n / 8 + n / 16 bytes (three bitmaps over the rows, the rank of one),
 * 8 nrec, per piece 8 (lo, mate) + 2 x 45 (masks, link, successor mark, chain minimum, two states of 16 bytes) + 3 / 16
 * bytes, 16 bytes per present node (two lists); a call that writes adds 48 bytes per unitig, seq_bytes, 32 bytes per
 * forward edge string (two key buffers of 2 x edge strings) + their bitmap, 8 bytes per edge and the radix workspace.
 * A failed allocation is DEBWT_ENOMEM and leaves the kept arrays as they were.
 *
 * Arrays, capacities, the sizing call and the return codes are those of debwt_fm_cdbg; DEBWT_EINVAL in addition for an even
 * k (debwt_fm_last_error says why) and for an index of 2^31 rows or more.  flags: none defined, must be 0. */
int debwt_fm_cdbg_both(debwt_fm *fm, uint32_t k, uint32_t flags, debwt_fm_unitig *unitigs, uint64_t unitig_capacity,
                       uint8_t *seq, uint64_t seq_capacity, debwt_fm_cdbg_edge *edges, uint64_t edge_capacity,
                       debwt_fm_cdbg_sizes *sizes);
/* what the last debwt_fm_cdbg_both did.  The counting fields of debwt_fm_cdbg_stats over reported unitigs and canonical
 * nodes: nodes (canonical k-mers), edge_strings (oriented edge strings = 2 links + edges), unitigs, circular, links (member
 * links of the reported unitigs), edges, longest_nodes, seq_bytes; present (nodes of S's forward graph), mated (present
 * nodes whose reverse complement is present too), hairpins; jump_rounds, jump_steps, jump_wave_steps as in
 * debwt_fm_cdbg_stats over the oriented ids; rank_lines (rank lines read for left counts), mate_steps (rank steps of the
 * mate search, at most k x present), edge_keys (keys sorted before equal neighbours were dropped; 0 for a sizing call),
 * scratch_bytes; ms per phase (events: nodes = bits, rank and lo; mates; links = masks and links; rank = the rounds;
 * write = minima, pairs, unitigs, strings and edges) and host wall time */
typedef struct {
    uint64_t nodes, edge_strings, unitigs, circular, links, edges, longest_nodes, seq_bytes, present, mated, hairpins,
        jump_rounds, jump_steps, jump_wave_steps, rank_lines, mate_steps, edge_keys, scratch_bytes;
    float ms_nodes, ms_mates, ms_links, ms_rank, ms_write, ms_wall;
} debwt_fm_cdbg_both_stats;
int debwt_fm_cdbg_both_stats_get(const debwt_fm *fm, debwt_fm_cdbg_both_stats *out);

/* ---- string graph of the indexed records (fm_graph_kernels.h) --------------------------------------------------------
 * Records S_0 .. S_{nrec-1} are those of the index, numbered as in overlap hits; |S| is the length of S.
 * 1. state[i] = 1 (duplicate) iff some j < i has S_j == S_i; otherwise 2 (contained) iff S_i is a substring of a strictly
 *    longer record (a prefix, a suffix or an inner part); otherwise 0 (kept).  States do not depend on min_overlap.
 * 2. E: for kept i and kept j != i, (i -> j, L) is in E iff L is the largest length with min_overlap <= L and
 *    S_i[|S_i| - L ..) == S_j[0 .. L): DEBWT_FM_OVERLAP_LONGEST per pair, strand 0, self overlaps dropped.  Both ends are
 *    kept, so L < min(|S_i|, |S_j|): DEBWT_EINTERNAL otherwise.  Out-list order per source: (L descending, record ascending).
 * 3. (i -> k, L_ik) in E is reducible iff some j outside {i, k} has (i -> j, L_ij) in E with L_ij > L_ik and (j -> k, L_jk)
 *    in E with L_jk == |S_j| - L_ij + L_ik.  E is read as it is before anything is removed.  The irreducible graph is E
 *    minus its reducible edges.  Where the longest j -> k overlap is longer than the one that fits (periodic reads) no
 *    witness is in E and the edge stays.
 * 4. Unitigs over the irreducible graph: u -> w is a link iff outdeg(u) == 1, w is u's only successor, indeg(w) == 1 and
 *    w != u.  A unitig is a maximal chain of links; a node with no incoming link starts one; a component in which every
 *    node has an incoming link is a cycle, which starts at its lowest record and is flagged circular.  Every kept node is
 *    in exactly one unitig, and unitigs are numbered by ascending first record.
 * Strand 0 only; for a read set sampled from both strands debwt_fm_string_graph_both (below) gives the strand-complete
 * graph from the same index.
 *
 * debwt_fm_string_graph writes state (nrec) and edge_offsets (nrec + 1) first, then the edges of the irreducible graph,
 * or of E with DEBWT_FM_GRAPH_ALL_EDGES; DEBWT_ERANGE when capacity < edge_offsets[nrec] (the protocol of
 * debwt_fm_locate; edges may be NULL then).  DEBWT_EINVAL for min_overlap 0 and unknown flags.  The records are read
 * from the attached text; an index without one restores it first (debwt_fm_restore_text), so an index from
 * debwt_fm_open answers as one from debwt_fm_create.  Only kept records are walked, in the batches of debwt_fm_overlaps
 * (DEBWT_FM_OVERLAP_SLOTS, DEBWT_FM_OVERLAP_HITS; the result depends on neither).  E stays in HBM, 8 bytes an edge, from
 * the walk to the reduction: DEBWT_ENOMEM with the edge count in debwt_fm_last_error when it does not fit. */
typedef struct { uint32_t record, length; } debwt_fm_edge;
#define DEBWT_FM_GRAPH_ALL_EDGES 1u    /* skip the reduction: return E */
int debwt_fm_string_graph(debwt_fm *fm, uint32_t min_overlap, uint32_t flags,
                          uint8_t *state /* nrec */, uint64_t *edge_offsets /* nrec + 1 */,
                          debwt_fm_edge *edges, uint64_t capacity);
/* Definition 3 on a caller's edge list, on the index's device and stream: keep[e] = 0 for a reducible edge, 1 otherwise.
 * Source i's edges are edges[edge_offsets[i] .. edge_offsets[i + 1]), lengths descending; edges of one length may stand in
 * any record order.  reclen[i] = |S_i|.  DEBWT_EINVAL with the reason in debwt_fm_last_error: decreasing offsets, a
 * target >= nnodes, a target equal to the source, lengths not descending inside a source, a target repeated inside a
 * source, L >= min(reclen[source], reclen[target]), nnodes of 2^32 or more. */
int debwt_fm_edges_reduce(debwt_fm *fm, const uint64_t *reclen, uint64_t nnodes,
                          const uint64_t *edge_offsets, const debwt_fm_edge *edges,
                          uint8_t *keep /* one byte per edge */);
/* Definition 4 on the host (no GPU), in time linear in nodes and edges.  Only nodes of state 0 take part; an edge from
 * or to another node is DEBWT_EINVAL, as are decreasing offsets and a target >= nnodes.  members holds every kept node
 * once, unitig u's in members[unitig_offsets[u] .. unitig_offsets[u + 1]) in path order; the first *nunitigs entries of
 * circular and *nunitigs + 1 of unitig_offsets are meaningful. */
int debwt_fm_unitigs(const uint8_t *state, const uint64_t *edge_offsets, const debwt_fm_edge *edges,
                     uint64_t nnodes, uint64_t *unitig_offsets /* nnodes + 1 */, uint32_t *members /* nnodes */,
                     uint8_t *circular /* nnodes */, uint64_t *nunitigs);
/* what the last debwt_fm_string_graph or debwt_fm_edges_reduce did: records, the three states, overlap hits walked, edges
 * of E, reducible edges, witness lists searched, kernel launches, the largest device scratch of a batch, the bytes of E
 * resident, and the time of the walk (state search, walk, compaction, expansion), of the edge build and of the reduction
 * (reduction and compaction of the kept edges), by events, and host wall time.  debwt_fm_edges_reduce fills records
 * (nnodes), edges, reducible, lookups, launches, edge_bytes, ms_reduce and ms_wall. */
typedef struct {
    uint64_t records, kept, duplicates, contained, hits, edges, reducible, lookups, launches, scratch_bytes, edge_bytes;
    float ms_walk, ms_build, ms_reduce, ms_wall;
} debwt_fm_graph_stats;
int debwt_fm_graph_stats_get(const debwt_fm *fm, debwt_fm_graph_stats *out);

/* ---- string graph over both strands (fm_bigraph_kernels.h) ------------------------------------------------------------
 * Let D = (S_0, rc S_0, S_1, rc S_1, ...) be the doubled collection: record 2r + o of D is the oriented node (r, o), o = 1
 * for the reverse complement.  The strand-complete graph of S is definitions 1-3 above applied to D, with node ids
 * 2r + o; D is never built, and the index is the one of S.  It follows that state[2r] is 1 iff some q < r has S_q == S_r
 * or S_q == rc S_r, else 2 iff S_r or rc S_r lies inside a strictly longer record, else 0; state[2r + 1] == state[2r]
 * unless S_r == rc S_r (a self-rc read), where state[2r + 1] == 1: node (r, -) of a kept self-rc read does not exist and
 * every relation that would name it names (r, +).  E and the irreducible graph are closed under u -> v  |->  v^1 -> u^1.
 * 2r -> 2r + 1 and 2r + 1 -> 2r (a read that overlaps its own reverse complement) are edges; only v -> v is dropped.
 * (i+ -> j+) and (i- -> j+) are the overlaps of debwt_fm_overlaps on strands 0 and 1; (i+ -> j-, L), where the last L
 * bases of S_i are the reverse complement of the last L of S_j, is found by locating rc(last min_overlap bases of S_i)
 * and comparing the rest in the attached text; (i- -> j-) is the mirror of (j+ -> i+).
 *
 * debwt_fm_string_graph_both writes state (2 nrec), edge_offsets (2 nrec + 1) and edges (.record = 2r + o) byte for byte
 * as debwt_fm_string_graph does on an index of D, with its capacity protocol (DEBWT_ERANGE), its restore of a missing
 * text and its DEBWT_ENOMEM.  DEBWT_EINVAL for min_overlap 0, flags other than DEBWT_FM_GRAPH_ALL_EDGES and 2^31 records
 * or more.  The walk and the located seed rows go in the batches of debwt_fm_overlaps (DEBWT_FM_OVERLAP_SLOTS,
 * DEBWT_FM_OVERLAP_HITS; the result depends on neither).  The work of the tail-to-tail search is the number of
 * occurrences of the min_overlap-long seeds, not the number of overlaps. */
int debwt_fm_string_graph_both(debwt_fm *fm, uint32_t min_overlap, uint32_t flags,
                               uint8_t *state /* 2 * nrec */, uint64_t *edge_offsets /* 2 * nrec + 1 */,
                               debwt_fm_edge *edges, uint64_t capacity);
/* 4b. Oriented unitigs on the host (no GPU), in linear time, over the irreducible graph of debwt_fm_string_graph_both
 * (nnodes = 2 nrec, even).  Read r is self-rc iff state[2r] == 0 and state[2r + 1] == 1.  u -> w is a link iff definition
 * 4 makes it one, w != u^1, and neither u nor w belongs to a self-rc read.  The unitigs of definition 4 under this rule
 * come in mirror pairs U, U' (U reversed, every member ^ 1; a mirror cycle rotated to its lowest member; the node of a
 * self-rc read is its own mirror).  Of each pair the one with the lower first member is reported, numbered by ascending
 * first member: every kept read is in exactly one reported unitig, in one orientation.  Arguments and errors as
 * debwt_fm_unitigs; an odd nnodes is DEBWT_EINVAL. */
int debwt_fm_unitigs_both(const uint8_t *state, const uint64_t *edge_offsets, const debwt_fm_edge *edges,
                          uint64_t nnodes, uint64_t *unitig_offsets /* nnodes + 1 */, uint32_t *members /* nnodes */,
                          uint8_t *circular /* nnodes */, uint64_t *nunitigs);
/* what the last debwt_fm_string_graph_both did.  The fields of debwt_fm_graph_stats, the three states counted in reads
 * (state[2r]); selfrc: kept self-rc reads; seeds: tail seeds searched, seed_rows: their occurrences located, tail_hits:
 * occurrences that verified; edges_kind: the edges of E that are ++, +-, -+, -- (source, target); ms_tail: seed, locate
 * and verify; ms_merge: the mirrors and the ordering of the lists; ms_walk, ms_build, ms_reduce, ms_wall as there. */
typedef struct {
    uint64_t records, kept, duplicates, contained, hits, edges, reducible, lookups, launches, scratch_bytes, edge_bytes;
    uint64_t selfrc, seeds, seed_rows, tail_hits, edges_kind[4];
    float ms_walk, ms_build, ms_reduce, ms_wall, ms_tail, ms_merge;
} debwt_fm_graph_both_stats;
int debwt_fm_graph_both_stats_get(const debwt_fm *fm, debwt_fm_graph_both_stats *out);

/* ---- graph cleaning: tips and bubbles (fm_clean_kernels.h) --------------------------------------------------------------
 * 6. Over nnodes nodes with state bytes and the CSR lists edge_offsets / edges, with max_tip T, max_bubble B, max_rounds R.
 *    A node is alive iff its state is 0.  Every phase works on a snapshot: out(v) and in(v) are the alive neighbours of an
 *    alive v through the edges as given (one entry per edge), every decision of a phase reads the snapshot, and the
 *    removals of a phase are applied together after it, so no result depends on an order of evaluation (as in 3).
 *    Tip phase.  For w with outdeg(w) >= 2 and each x in out(w), follow the chain c_1 = x, c_2, ...: the edge is a tip iff
 *    some m <= T has indeg(c_t) == 1 for every t <= m, outdeg(c_t) == 1 with c_{t+1} its successor for t < m, and
 *    outdeg(c_m) == 0.  If at least one out-edge of w is no tip, the chains of all its tip edges are removed (c_1 .. c_m
 *    get state 3, clipped); if every out-edge of w is a tip, nothing of w is removed.  The same rule runs on the transposed
 *    snapshot (backward tips into a w with indeg(w) >= 2); both directions read one snapshot and their removals are
 *    united.  No node is in a tip of either kind twice: a forward tip's nodes have indeg 1, so one edge leads into its
 *    chain, and a backward tip's far end has indeg 0.
 *    Bubble phase, on a new snapshot taken after the tip removals.  For w with outdeg(w) >= 2 and each x in out(w), walk
 *    c_1 = x, c_2, ... while indeg(c) == 1 and outdeg(c) == 1, at most B nodes.  The walk yields a simple branch (a chain
 *    of m >= 1 nodes and its end z) iff it stops at a node z with indeg(z) >= 2 and z != w; it yields none when
 *    indeg(x) >= 2 (m == 0), when a chain node has outdeg != 1, and when it would need more than B nodes.  The simple
 *    branches of w are grouped by z; a group of two or more is ranked by (m descending, key ascending), key being the
 *    least node of the chain, or with DEBWT_FM_CLEAN_MIRRORED the least v >> 1, so that a mirrored bubble gets one verdict
 *    from both ends.  If the best rank is held by one branch, the chains of all others of the group are removed (state 4,
 *    popped); if two branches tie for it on m and key, nothing of the group is removed.
 *    One round is a tip phase, then a bubble phase; rounds repeat until one removes nothing or R have run.  Every walk is
 *    bounded by T or B, so cycles end.  With T == 0 there is no tip phase, with B == 0 no bubble phase.
 * state_out is state with 3 and 4 written in; edge_keep[e] (indexed as edges) is 1 iff both ends of edge e are alive at
 * the end.  With DEBWT_FM_CLEAN_MIRRORED (node ids 2r + o, as from debwt_fm_string_graph_both) and lists closed under
 * u -> v  |->  v^1 -> u^1 the result is closed too: state_out[v] == 0 iff state_out[v ^ 1] == 0, but for the second node
 * of a self-rc read.  Edge lengths are not read.  The lists are uploaded once and transposed once on the index's device
 * and stream; a round changes states and counters only.
 * DEBWT_EINVAL with the reason in debwt_fm_last_error: T == 0 and B == 0 together, R == 0, unknown flags, decreasing
 * offsets, a target >= nnodes, an edge from or to a node that is not alive, an odd nnodes with DEBWT_FM_CLEAN_MIRRORED,
 * nnodes of 2^32 or more.
 * Not done here: isolated short unitigs stay (a read with an error in its middle has no overlap of min_overlap and stands
 * alone), no edge is cut by its overlap ratio, and a bubble whose branches branch themselves is not popped. */
#define DEBWT_FM_CLEAN_MIRRORED 1u
#define DEBWT_FM_NODE_CLIPPED 3
#define DEBWT_FM_NODE_POPPED 4
typedef struct { uint32_t max_tip, max_bubble, max_rounds, flags; } debwt_fm_clean_opts;
/* max_tip 4, max_bubble 16, max_rounds 8, no flags */
void debwt_fm_clean_defaults(debwt_fm_clean_opts *o);
int debwt_fm_graph_clean(debwt_fm *fm, const uint8_t *state, const uint64_t *edge_offsets, const debwt_fm_edge *edges,
                         uint64_t nnodes, const debwt_fm_clean_opts *opts, uint8_t *state_out /* nnodes */,
                         uint8_t *edge_keep /* one byte per edge */);
/* The edges with keep[e] != 0, on the host (no GPU), order kept: offsets_out (nnodes + 1, from 0) and edges_out.
 * DEBWT_EINVAL for decreasing offsets and a NULL array. */
int debwt_fm_edges_compact(const uint64_t *edge_offsets, const debwt_fm_edge *edges, const uint8_t *keep, uint64_t nnodes,
                           uint64_t *offsets_out, debwt_fm_edge *edges_out);
/* what the last debwt_fm_graph_clean did: nodes and edges given, rounds run (the one that removed nothing included), tip
 * chains clipped and their nodes, branches popped and their nodes (a tie group that stays counts nothing), nodes visited
 * by the walks, kernel launches, the time of the kernels (transpose included) by events, and host wall time */
typedef struct {
    uint64_t nodes, edges, rounds, tips, tip_nodes, bubbles, bubble_nodes, steps, launches;
    float ms_clean, ms_wall;
} debwt_fm_clean_stats;
int debwt_fm_clean_stats_get(const debwt_fm *fm, debwt_fm_clean_stats *out);

/* ---- pileup of alignments, calls and consensus (fm_pile_kernels.h) ---------------------------------------------------
 * Definition 7 (pileup).  Input: the reads as the mapper takes them (patterns / offsets / npat; offsets[0] need not be 0,
 * so a caller can pass a run of reads of a larger set: only patterns[offsets[0] .. offsets[npat]) is uploaded); naln alignments, each a
 * debwt_fm_pile_aln {pattern, tbeg, qbeg, strand}; their CIGARs through cigar_offsets (naln + 1) and cigar, BAM-coded
 * (len << 4 | op, M 0, I 1, D 2) exactly as debwt_fm_extend, debwt_fm_map, debwt_fm_map_chained and debwt_fm_map_pairs
 * return them; a window [wbeg, wend) of global text positions.
 *    Query string.  Q is the pattern (strand 0) or its reverse complement (strand 1); qbeg is a coordinate in Q, as in
 *    debwt_fm_extend.  The CIGAR reads left to right along the text, from query index qbeg and text position tbeg.
 *    Events.  Each adds 1 to counts[t - wbeg][slot], and only when wbeg <= t < wend:
 *      a column of an M op at (i, t): the code of Q[i] is the slot, A 0, C 1, G 2, T 3 (either case); any other
 *      character goes to slot 6;
 *      every text position t of a D op: slot 4;
 *      an I op: slot 5 at t = (text position of the next text-consuming column) - 1, the last base before the insertion.
 *    Slot 7 is never written: the stride of 8 uint32_t keeps a position at 32 bytes.
 *    Validity.  An alignment with an empty CIGAR contributes nothing.  DEBWT_EINVAL, with nothing counted and the table
 *    as it was, for: an op code above 2; an op of length 0; a CIGAR whose first or last op is not M; pattern >= npat;
 *    strand > 1; qbeg + the consumed query bases > the read's length; tbeg + the consumed text > n; wend <= wbeg or
 *    wend > n; decreasing cigar_offsets.  (A first or last op that is a gap has no anchor -- an insertion before tbeg
 *    would count at tbeg - 1, outside the alignment -- and the local recurrence of debwt_fm_extend never returns one: a
 *    gap costs o + e > 0, so an optimal local alignment that began or ended with one would score more without it.)
 *    Alignments are not checked against record boundaries.
 * The table stays in HBM, owned by the index, as the attached text is (32 bytes x the window, counted in
 * debwt_fm_info.device_bytes; DEBWT_ENOMEM when it does not fit).  Without DEBWT_FM_PILE_ADD a call clears the table
 * first; with it the call adds to the resident table, which must be of the same window (DEBWT_EINVAL otherwise; with no
 * table resident the flag changes nothing), so reads can arrive in batches: the result does not depend on the batching.
 * Counts are 32-bit and wrap at 2^32 adds to one slot.  DEBWT_PILE_FORM (environment, read per call): "lane" counts with
 * one lane per alignment instead of a group of lanes per alignment; the tables are identical. */
#define DEBWT_FM_PILE_ADD 1u
typedef struct { uint64_t pattern; uint64_t tbeg; uint32_t qbeg, strand; } debwt_fm_pile_aln;
int debwt_fm_pileup(debwt_fm *fm, const char *patterns, const uint64_t *offsets, uint64_t npat,
                    const debwt_fm_pile_aln *alns, uint64_t naln, const uint64_t *cigar_offsets, const uint32_t *cigar,
                    uint64_t wbeg, uint64_t wend, uint32_t flags);
/* the resident table to the host: window[0] = wbeg, window[1] = wend (written first), counts 8 words per position;
 * DEBWT_ERANGE when capacity (in positions) is below wend - wbeg, DEBWT_ESTATE without a table */
int debwt_fm_pile_fetch(debwt_fm *fm, uint64_t *window, uint32_t *counts, uint64_t capacity);
/* frees the table; DEBWT_OK when there is none */
int debwt_fm_pile_release(debwt_fm *fm);
/* Definition 8 (calls), on the resident table (DEBWT_ESTATE without one).  The text is restored first when the index has
 * none (debwt_fm_restore_text).
 *    ref[t]: the text's base code 0..3, or 4 at a position that holds no base of a record (separators, end marker).
 *    Depth d = counts[0] + ... + counts[4]; slot 6 is ignored.
 *    best = the slot in 0..4 with the largest count; on a tie ref[t] when ref[t] is among the tied slots, else the lowest.
 *    A position is called iff ref[t] != 4, d >= min_depth and counts[best] * 1000 >= min_permille * d.
 *    calls[t - wbeg] = best for a called position, 5 otherwise; bit 0x10 is set when the position is called and
 *    counts[5] * 1000 >= min_permille * d.
 *    Variants: the called positions with best != ref[t] or bit 0x10, in ascending t; depth = d (saturated at 2^32 - 1),
 *    count = counts[best], ins = counts[5], call = the call byte.
 * calls (wend - wbeg bytes) and ref (the same; may be NULL) are written first, then *nvars = the number of variants;
 * DEBWT_ERANGE when capacity is below it.  opts NULL: the defaults, min_depth 4 and min_permille 600 -- knobs chosen by
 * hand, not measurements: a majority of 60 % of at least 4 reads. */
typedef struct { uint32_t min_depth, min_permille; } debwt_fm_pile_opts;
typedef struct { uint64_t t; uint32_t depth, count, ins; uint8_t ref, call; } debwt_fm_variant;
void debwt_fm_pile_defaults(debwt_fm_pile_opts *opts);
int debwt_fm_pile_call(debwt_fm *fm, const debwt_fm_pile_opts *opts, uint8_t *calls, uint8_t *ref,
                       debwt_fm_variant *variants, uint64_t capacity, uint64_t *nvars);
/* The insertions behind the counts of slot 5: one event per I op of the alignments (as given to debwt_fm_pileup; the same
 * validity) that is anchored at one of `positions` (npos of them, strictly ascending: normally the variants with bit
 * 0x10).  qpos: the query index in Q of the first inserted base, len: the op's length, aln: the alignment.  Events are
 * ordered by (t, aln, qpos).  *nevents is written first; DEBWT_ERANGE when capacity is below it.  No table is needed. */
typedef struct { uint64_t t, aln; uint32_t qpos, len; } debwt_fm_ins_event;
int debwt_fm_pile_insertions(debwt_fm *fm, uint64_t npat, const uint64_t *offsets, const debwt_fm_pile_aln *alns, uint64_t naln,
                             const uint64_t *cigar_offsets, const uint32_t *cigar, const uint64_t *positions, uint64_t npos,
                             debwt_fm_ins_event *events, uint64_t capacity, uint64_t *nevents);
/* The vote over the events of ONE position (host only, no GPU).  The string of an event is Q[qpos, qpos + len) of its
 * alignment written with A, C, G, T and N for any other character.  The most frequent string wins; ties go to the shorter
 * string, then to the lexicographically smaller.  out receives it without a terminator, *len its length (written first;
 * DEBWT_ERANGE when capacity is below it), *support its number of events.  No events: length 0, support 0.
 * DEBWT_EINVAL for an event that names an alignment >= naln or bases outside its read. */
int debwt_fm_ins_vote(const char *patterns, const uint64_t *offsets, uint64_t npat, const debwt_fm_pile_aln *alns, uint64_t naln,
                      const debwt_fm_ins_event *events, uint64_t nevents, char *out, uint64_t capacity, uint64_t *len,
                      uint32_t *support);
/* The consensus of every record inside a window (host only, no GPU).  ref and calls: wend - wbeg bytes as
 * debwt_fm_pile_call wrote them.  Insertions: nins voted strings, insertion i anchored at ins_t[i] (ascending), its bases
 * ins_bases[ins_offsets[i] .. ins_offsets[i + 1]), its support and the depth of its position.  rec_starts (nrec,
 * ascending; the text has n positions) as debwt_fm_record_starts gives them.  Per position of a record inside the window:
 * the called base in upper case; the reference base in lower case where no call was made; nothing for a called deletion;
 * then, at a position with bit 0x10 that has a voted string with support * 1000 >= min_permille * depth, that string.
 * out_offsets (nrec + 1) is written first: record r's consensus is out[out_offsets[r] .. out_offsets[r + 1]), empty for a
 * record outside the window.  DEBWT_ERANGE when capacity < out_offsets[nrec]. */
int debwt_fm_consensus(const uint8_t *ref, const uint8_t *calls, uint64_t wbeg, uint64_t wend, const uint64_t *ins_t,
                       const uint64_t *ins_offsets, const char *ins_bases, const uint32_t *ins_support,
                       const uint32_t *ins_depth, uint64_t nins, uint32_t min_permille, const uint64_t *rec_starts,
                       uint64_t nrec, uint64_t n, uint64_t *out_offsets, char *out, uint64_t capacity);
/* what the last debwt_fm_pileup did (alignments, ops, and the input's M columns, D bases and I ops; the adds made inside
 * the window by kind: bases, other characters, deletions, insertions; kernel launches; group: lanes per alignment of the
 * counting kernel, 1 for the lane form; the table's bytes; kernel time by events of the validity pass and of the counting
 * kernel; host wall time), and the last debwt_fm_pile_call (positions, variants, kernel time, wall time) */
typedef struct {
    uint64_t alignments, ops, m_columns, d_bases, i_ops, ev_base, ev_other, ev_del, ev_ins, launches, group, table_bytes;
    uint64_t call_positions, call_variants;
    float ms_plan, ms_kernel, ms_wall, ms_call, ms_call_wall;
} debwt_fm_pile_stats;
int debwt_fm_pile_stats_get(const debwt_fm *fm, debwt_fm_pile_stats *out);

void debwt_fm_destroy(debwt_fm *fm);

#ifdef __cplusplus
}
#endif
#endif
