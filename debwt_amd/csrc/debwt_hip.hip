// debwt_hip.hip -- C ABI (include/debwt_hip.h) and stage orchestration of the gfx950 deBWT path.
//
// One context = one GPU = one HIP stream.  Device buffers grow on demand and are kept between runs,
// so a steady-state run performs no allocation.  The only host work inside a run is the
// special-region module (special_host.cpp), which overlaps the GPU's key sort.
#include "../../include/debwt_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "radix_sort.h"
#include "special_host.h"
#include "fasta_host.h"
#include "gz_parallel.h"
#include "stage_kernels.h"
#include "special_kernels.h"
#include "verify_kernels.h"
#include "fm_kernels.h"
#include "fm_search_kernels.h"
#include "fm_mem_kernels.h"
#include "fm_extend_kernels.h"
#include "fm_chain_kernels.h"
#include "fm_window_kernels.h"
#include "fm_overlap_kernels.h"
#include "fm_overlap_mm_kernels.h"
#include "fm_extract_kernels.h"
#include "fm_esa_kernels.h"
#include "fm_repeat_kernels.h"
#include "fm_record_kernels.h"
#include "fm_cdbg_kernels.h"
#include "fm_bicdbg_kernels.h"
#include "fm_kmer_kernels.h"
#include "fm_spectrum_kernels.h"
#include "fm_graph_kernels.h"
#include "fm_bigraph_kernels.h"
#include "fm_clean_kernels.h"
#include "fm_pile_kernels.h"

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

enum Stage { ST_EMPTY = 0, ST_LOADED, ST_SORTED, ST_CLASSIFIED, ST_SP, ST_BLUE, ST_ASSEMBLED };

}  // namespace

struct debwt_ctx {
    debwt_config cfg{};
    int K = 31;
    hipStream_t stream = nullptr;
    std::string err;
    Stage stage = ST_EMPTY;
    debwt_stats st{};

    // host side of the loaded text
    const uint64_t *h_text = nullptr;
    std::vector<uint64_t> own_text;
    std::vector<uint64_t> h_sep;
    uint64_t n = 0, nrec = 0, M = 0, NS = 0;
    SpecialTables special;

    // device buffers
    DevBuf rs_rle, text, sepbits, sep, keysA, keysB, rs_counts, cp_counts, dk, dstart, mchar, head_keys, facts, facts_tmp,
        red, red_q, mi_j0, mi_freq, bstart, cursor, blue, spkey, sprow, spchr, branch, pflag, spsym, spn, bwt,
        hmask, hash_rows, dollar, large_q, large_k0, large_en, rowsym, momask, mimask, rbits, rs_over, rs_skew, rs_pair, mi_list, htab, fact_work, facts_all, shard_hist, dest_tab, qbounds, qcursor, qlist, qwave;
    DevBuf brbits;              // the special branches as a bitmap over the text positions (collections of many records)
    DevBuf blue_done;           // one byte per multi-in block: finished by k_blue_classify
    bool branch_bitmap = false;
    DevBuf sx, sppos, sprec, tail_d;   // special-region module on the device: scratch arena, positions / records of the sorted items, tail facts
    bool special_dev = false;   // the tables of this build were made on the device (spkey / spchr / branch / head_keys / tail_d)
    u64 nbranch = 0;            // special branches (specialBranchNum)
    u32 *h_over = nullptr;      // pinned mirror of rs_over
    u64 *sk = nullptr;          // sorted keys (keysA or keysB)
    u32 *h_scalars = nullptr;   // pinned read-back area
    u64 D = 0, Q = 0, Rmo = 0, R = 0, B = 0, S = 0, nlarge = 0, nfacts = 0;
    u64 rQ = 0, rB = 0, rnlarge = 0;   // blocks, blue rows, large blocks of the range just classified
    u64 rn1024 = 0, n1024 = 0;         // blocks of 513..1024 rows (range / context)
    u64 rn512 = 0, n512 = 0;           // blocks of 257..512 rows
    // Key ranges of this context, sorted and classified one after the other over the resident text (one range unless
    // the node instances exceed range_cap: "bucket streaming" for texts whose keys do not fit HBM at once).
    // D, Rmo and the buffers keysA/keysB/dk/dstart/pflag/mi_*/bstart/facts belong to the range being processed;
    // Q, B, nlarge and blk_*/facts_acc/large_q/mchar/sprow cover the whole context with 64-bit offsets.
    struct KeyRange { u64 key_lo, key_hi, M, Mbase, Q, qbase, B, Bbase, s0, s1, l0, nl;      // l0, nl: its blocks above the LDS capacity in large_q
                      bool heavy = false, heavy_known = false; };   // heavy: long 12-mer bins, no bucket pass (heavy_ranges)
    std::vector<KeyRange> ranges;
    u64 range_cap = 0;          // 0: from the free HBM at the first build (plan_ranges)
    u64 Mctx = 0;               // node instances of this context (sum over its ranges)
    u64 nfacts_acc = 0;         // facts accumulated over the ranges
    bool local_done = false;    // classify_local already ran per range (multi-range build)
    bool plan_valid = false;    // `ranges` holds the cuts of the loaded text (several ranges)
    DevBuf vidx, vtmp;          // debwt_verify_device: rank structure (when no free key buffer holds it), small arrays
    DevBuf ls_buf, blk_j0, blk_freq, blk_start, facts_acc, large_tmp, blue_tmp, sub_start, sub_j0, sub_freq, sub_depth, range_hist;
    // k-mer-prefix shard of a multi-GPU build (world == 1: the whole key space)
    int shard_rank = 0, shard_world = 1;
    u64 Mfull = 0;              // node instances of the whole text
    u64 key_lo = 0, key_hi = 0; // this shard's key range [lo, hi); hi == 0: unbounded
    u64 Mbase = 0;              // node instances in the shards before this one
    u64 qbase = 0;              // multi-in blocks in the shards before this one
    u64 Btotal = 0;             // multi-in positions of the whole text
    u64 s0 = 0, s1 = 0;         // special suffixes [s0, s1) fall into this shard's node range
    bool facts_ready = false;
    u64 n_hash_local = 0;
    bool route_direct = false;  // SP pass 1 keeps the block ids of the multi-in positions (qlist: one run per wave, found
    u64 gq0 = 0;                //   through qwave, group gq0 first; qwave[0] is the bump counter), pass 2 writes routed entries
    bool exchange = false;      // sharded exchange mode: the keys of every range arrive by alltoallv in a caller buffer
    bool whole_build = false;   // inside debwt_build / debwt_build_to_host: nothing between the stages can be fetched
    bool shard_planned = false; // `ranges` were cut by debwt_shard_plan from the global census
    u64 *sort_a = nullptr, *sort_b = nullptr;   // the two key buffers of the range being sorted
    u64 Dsum = 0;               // distinct keys over the ranges sorted so far
    bool shared_hist = false;   // the first-pass histograms of all ranges came from one scan of the text
    u64 Qtotal = 0;             // multi-in blocks of the whole text (all shards)
    u64 S_rank = 0, B_rank = 0; // SP symbols / multi-in positions of this shard's text slice (all its sub-slices)
    bool reclaim_ok = false;    // an allocation that fails may release the idle buffers of the other stages (reclaim)
    u64 *routed = nullptr;      // ... and its routed blue entries (debwt_shard_sp_emit): a key buffer when one is free, else facts_tmp
    struct SubSlice { u64 g0, g1, S, B; };
    std::vector<SubSlice> sub;  // the slice in pieces of < 2^32 positions
    std::thread special_thread; // host special-region module, runs beside the key sort of the first range
    bool special_running = false;
    u64 g0 = 0, g1 = 0;         // text slice of this shard for the SP stage, in 32-position groups
    u64 S_local = 0, B_slice = 0, sp_off = 0;
    int hbits = 10, pbits = 13;
    bool mzfilter = false;      // the prefilter is indexed by the nodes' minimizers (pbits = log2 of its 64-bit words)
    int mzw = 16;               // ... of this many symbols
    bool mztable = false;       // ... and so is the node table (k_build_hash)
    bool abs32 = true;          // fill cursors hold absolute blue slots

    hipStream_t copy_stream = nullptr;   // debwt_build_to_host: finished row ranges leave on this stream under the blue sort
    hipEvent_t ev_copy = nullptr, ev_copy2 = nullptr;
    std::vector<u64> census;             // 12-mer prefix census of the loaded text, taken piece by piece behind its upload
    bool census_valid = false;
    hipEvent_t ev[8]{};         // stage boundaries
    hipEvent_t ev_pass[16][2]{};
    int n_pass_events = 0;
};

namespace {

#define HIPCHK(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
            return e_ == hipErrorOutOfMemory ? DEBWT_ENOMEM : DEBWT_EDEVICE;                   \
        }                                                                                      \
    } while (0)

// Out of memory inside a build: the buffers of the stages that are over (or have not begun) hold nothing the build still
// needs -- after the classification the workspace of the key ranges (key buffers, distinct keys, their first rows: 30 bytes per
// key), during the key sort what the SP stage and the blue sort of the build BEFORE left behind (node table, work lists,
// split scratch) -- and are released, largest users first, before the allocation is tried once more.  k = 16 on a 3.1 Gbp text
// (1.07 G branching 15-mers: a 64 GB node table, 3 G blue rows) builds this way on one GPU; a text that fits keeps every
// buffer from build to build as before.  Returns the bytes released.
// Only at the two points where no pointer into those buffers is held and every one of them is allocated again before its
// next use (reclaim_ok): the allocations at the start of the key sort and at the start of the SP stage.
size_t reclaim(debwt_ctx *c, const DevBuf *keep) {
    if (!c->reclaim_ok) return 0;
    std::vector<DevBuf *> idle;
    if (c->stage >= ST_CLASSIFIED) {
        idle = {&c->keysB, &c->dk, &c->dstart, &c->rs_rle, &c->pflag};
        if (!c->exchange) idle.push_back(&c->keysA);
        c->sk = nullptr; c->routed = nullptr;
    } else {
        idle = {&c->htab, &c->mi_list, &c->qlist, &c->qwave, &c->blue_tmp, &c->ls_buf, &c->vidx, &c->vtmp, &c->large_k0,
                &c->large_en, &c->rowsym, &c->spn, &c->spsym, &c->rbits, &c->blue, &c->momask, &c->mimask};
    }
    size_t freed = 0;
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf *b : idle)
        if (b != keep && b->p) { freed += b->cap; (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    if (getenv("DEBWT_TRACE_ALLOC")) fprintf(stderr, "reclaim: %.2f GB of idle buffers released\n", freed / 1e9);
    return freed;
}

int ensure(debwt_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return DEBWT_OK;
    static const bool trace = getenv("DEBWT_TRACE_ALLOC") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t old = b.cap;
    if (b.p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    const auto t1 = std::chrono::steady_clock::now();
    size_t want = bytes + bytes / 16 + 256;
    hipError_t me = hipMalloc(&b.p, want);
    if (me == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        b.p = nullptr;
        if (reclaim(c, &b)) me = hipMalloc(&b.p, want);
        if (me == hipErrorOutOfMemory) { (void)hipGetLastError(); want = bytes + 256; me = hipMalloc(&b.p, want); }   // without the slack
    }
    if (me != hipSuccess) { b.p = nullptr; c->err = std::string("hipMalloc of ") + std::to_string(want) + " bytes: " + hipGetErrorString(me); return me == hipErrorOutOfMemory ? DEBWT_ENOMEM : DEBWT_EDEVICE; }
    b.cap = want;
    if (trace && want > (64u << 20))
        fprintf(stderr, "ensure: %.2f GB (was %.2f): sync+free %.1f ms, malloc %.1f ms\n", want / 1e9, old / 1e9,
                std::chrono::duration<float, std::milli>(t1 - t0).count(),
                std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t1).count());
    return DEBWT_OK;
}
#define ENSURE(c, b, bytes) do { int r_ = ensure((c), (b), (bytes)); if (r_) return r_; } while (0)
// grows a buffer that accumulates over the key ranges: the first `used` bytes survive
int ensure_keep(debwt_ctx *c, DevBuf &b, size_t bytes, size_t used) {
    if (bytes <= b.cap) return DEBWT_OK;
    size_t want = bytes + bytes / 2 + 256;
    void *np = nullptr;
    HIPCHK(c, hipMalloc(&np, want));
    if (b.p) {
        if (used) HIPCHK(c, hipMemcpyAsync(np, b.p, used, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(b.p));
    }
    b.p = np; b.cap = want;
    return DEBWT_OK;
}
#define ENSURE_KEEP(c, b, bytes, used) do { int r_ = ensure_keep((c), (b), (bytes), (used)); if (r_) return r_; } while (0)

void plan_chunks(u64 n, u32 *nchunks, u64 *chunk) {
    const u64 DEBWT_TILE = (u64)DEBWT_BLOCK * CP_VEC;
    u64 tiles = (n + DEBWT_TILE - 1) / DEBWT_TILE;
    u64 c = tiles < CP_MAXCHUNKS ? tiles : CP_MAXCHUNKS;
    if (c == 0) c = 1;
    u64 per = (tiles + c - 1) / c;
    if (per == 0) per = 1;                              // n == 0: one empty chunk
    *chunk = per * DEBWT_TILE;
    *nchunks = (u32)((n + *chunk - 1) / *chunk);
    if (*nchunks == 0) *nchunks = 1;
}

// count + scan of a functor; the total lands in h_scalars[slot] once the stream is synchronised
template <class F> int cp_count(debwt_ctx *c, const F &f, u64 n, u32 *counts, int slot) {
    u32 nchunks; u64 chunk;
    plan_chunks(n, &nchunks, &chunk);
    if (n) cp_count_kernel<F><<<nchunks, DEBWT_BLOCK, 0, c->stream>>>(f, n, chunk, counts);
    else HIPCHK(c, hipMemsetAsync(counts, 0, sizeof(u32), c->stream));
    u32 *total = counts + CP_MAXCHUNKS;
    cp_scan_kernel<<<1, 1024, 0, c->stream>>>(counts, n ? nchunks : 1, total);
    HIPCHK(c, hipMemcpyAsync(&c->h_scalars[slot], total, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    return DEBWT_OK;
}
template <class F> int cp_count2(debwt_ctx *c, const F &f, u64 n, u32 *ca, int slot_a, u32 *cb, int slot_b) {
    u32 nchunks; u64 chunk;
    plan_chunks(n, &nchunks, &chunk);
    if (n) cp_count2_kernel<F><<<nchunks, DEBWT_BLOCK, 0, c->stream>>>(f, n, chunk, ca, cb);
    else { HIPCHK(c, hipMemsetAsync(ca, 0, sizeof(u32), c->stream)); HIPCHK(c, hipMemsetAsync(cb, 0, sizeof(u32), c->stream)); }
    cp_scan_kernel<<<1, 1024, 0, c->stream>>>(ca, n ? nchunks : 1, ca + CP_MAXCHUNKS);
    cp_scan_kernel<<<1, 1024, 0, c->stream>>>(cb, n ? nchunks : 1, cb + CP_MAXCHUNKS);
    HIPCHK(c, hipMemcpyAsync(&c->h_scalars[slot_a], ca + CP_MAXCHUNKS, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->h_scalars[slot_b], cb + CP_MAXCHUNKS, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    return DEBWT_OK;
}
template <class F> int cp_emit(debwt_ctx *c, const F &f, u64 n, const u32 *counts) {
    if (!n) return DEBWT_OK;
    u32 nchunks; u64 chunk;
    plan_chunks(n, &nchunks, &chunk);
    cp_emit_kernel<F><<<nchunks, DEBWT_BLOCK, 0, c->stream>>>(f, n, chunk, counts);
    return DEBWT_OK;
}
// each in-flight compaction needs its own counts area: CP_MAXCHUNKS + 1 words per slot
u32 *cp_area(debwt_ctx *c, int slot) { return c->cp_counts.as<u32>() + (size_t)slot * (CP_MAXCHUNKS + 16); }

int sync_check(debwt_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return DEBWT_OK;
}

// Copies between a CALLER's host buffer and the device are queued on the context's streams: whoever returns early with an
// error must not leave them in flight -- the caller is free to release the buffer as soon as the call is back.
struct DrainOnError {
    debwt_ctx *c;
    bool armed = true;
    ~DrainOnError() {
        if (!armed) return;
        if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
    }
};

inline u32 grid_for(u64 n, u32 block) { return (u32)((n + block - 1) / block); }

RadixWorkspace radix_ws(debwt_ctx *c) {
    RadixWorkspace ws{};
    ws.counts = c->rs_counts.as<u32>();
    ws.over = c->rs_over.as<u32>();
    ws.h_over = c->h_over;
    ws.over_cap = c->rs_over.cap >= 48 ? (u32)std::min<size_t>((c->rs_over.cap - 32) / 16, 0xFFFFFFFFu) : 0;
    ws.skew_list = c->rs_skew.as<u32>();
    ws.pair = c->rs_pair.as<u32>();                          // grown by whoever sorts enough keys to gain from it
    ws.pair_cap = c->rs_pair.cap;
    return ws;
}

// main: the key sort of a range (kernels named for the profile, keys possibly read off the text); otherwise one of
// the small auxiliary sorts.  Pass events are recorded when `record_passes`.
int sort_keys(debwt_ctx *c, u64 *a, u64 *b, u64 count, int key_bits, u64 **result, bool record_passes,
              const TextKeySrc *text = nullptr, bool main_sort = false, RleSink *sink = nullptr, const u64 *key_range = nullptr,
              bool heavy = false) {
    ENSURE(c, c->rs_over, radix_over_bytes(count));      // one list entry per 4096-key tile can be oversize
    // the joint counts of the last two array passes of a key range (no bytes unless the range's top byte is narrow)
    const u64 text_range[2] = {text ? text->key_lo : 0ull, text ? text->key_hi : 0ull};
    if (!key_range && text) key_range = text_range;
    ENSURE(c, c->rs_pair, radix_pair_bytes_u64(count, key_bits, key_range, heavy));
    RadixWorkspace ws = radix_ws(c);
    hipError_t e = hipSuccess;
    const bool main = main_sort || record_passes;
    const int net = (c->cfg.reserved & 32768) ? 32 : 0;     // bit 15: the bucket finish prefers the 4096-key network (tests)
    if (record_passes) {
        *result = radix_sort_u64(c->stream, a, b, count, key_bits, ws, c->cfg.sort_algo | net, &c->ev_pass[0][0], 16,
                                 &c->n_pass_events, &e, text, sink, key_range, heavy);
        c->st.radix_pass_keys = count;
    } else {
        *result = radix_sort_u64(c->stream, a, b, count, key_bits, ws, c->cfg.sort_algo | net | (main ? 0 : 16), nullptr, 0,
                                 nullptr, &e, text, sink, key_range, heavy);
    }
    if (e != hipSuccess) { c->err = std::string("radix sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
    return DEBWT_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------

// every device buffer of a context (all grow on demand and are reused by the next build)
static std::vector<DevBuf *> all_buffers(debwt_ctx *c) {
    return {&c->text, &c->sepbits, &c->sep, &c->keysA, &c->keysB, &c->rs_counts, &c->cp_counts, &c->dk,
            &c->dstart, &c->mchar, &c->head_keys, &c->facts, &c->facts_tmp, &c->red, &c->red_q,
            &c->mi_j0, &c->mi_freq, &c->bstart, &c->cursor, &c->blue, &c->spkey, &c->sprow, &c->spchr,
            &c->branch, &c->pflag, &c->spsym, &c->spn, &c->bwt, &c->hmask, &c->hash_rows, &c->dollar,
            &c->large_q, &c->large_k0, &c->large_en, &c->rowsym, &c->momask, &c->mimask, &c->rbits, &c->rs_over, &c->rs_skew, &c->rs_pair,
            &c->mi_list, &c->htab, &c->fact_work, &c->facts_all, &c->shard_hist, &c->dest_tab, &c->qbounds, &c->qcursor,
            &c->sx, &c->sppos, &c->sprec, &c->tail_d, &c->brbits,
            &c->blk_j0, &c->blk_freq, &c->blk_start, &c->facts_acc, &c->large_tmp, &c->blue_tmp, &c->sub_start, &c->sub_j0,
            &c->sub_freq, &c->sub_depth, &c->range_hist, &c->rs_rle, &c->ls_buf, &c->vidx, &c->vtmp, &c->qlist, &c->qwave,
            &c->blue_done};
}

extern "C" const char *debwt_strerror(int code) {
    switch (code) {
        case DEBWT_OK: return "ok";
        case DEBWT_EINVAL: return "invalid argument";
        case DEBWT_ENOMEM: return "out of memory";
        case DEBWT_EDEVICE: return "HIP runtime error";
        case DEBWT_ESTATE: return "stage called out of order";
        case DEBWT_ERANGE: return "input exceeds a capacity of this build";
        case DEBWT_EINTERNAL: return "internal consistency check failed";
        case DEBWT_EIO: return "file could not be written";
        default: return "unknown error";
    }
}

extern "C" const char *debwt_last_error(const debwt_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

extern "C" int debwt_get_config(const debwt_ctx *ctx, debwt_config *out) {
    if (!ctx || !out) return DEBWT_EINVAL;
    *out = ctx->cfg;
    return DEBWT_OK;
}

extern "C" int debwt_create(const debwt_config *cfg, debwt_ctx **out) {
    if (!cfg || !out || cfg->k < 12 || cfg->k > 32) return DEBWT_EINVAL;   // src/main.c:41-47
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) return DEBWT_EDEVICE;
    debwt_ctx *c = new (std::nothrow) debwt_ctx();
    if (!c) return DEBWT_ENOMEM;
    c->cfg = *cfg;
    if (c->cfg.sort_algo == 0) c->cfg.sort_algo = 3;
    c->K = cfg->k - 1;
    int rc = DEBWT_OK;
    auto fail = [&](int code) { debwt_destroy(c); return code; };
    if (hipSetDevice(cfg->device) != hipSuccess) return fail(DEBWT_EDEVICE);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return fail(DEBWT_EDEVICE);
    if (hipHostMalloc((void **)&c->h_scalars, 64 * sizeof(u32), hipHostMallocDefault) != hipSuccess)
        return fail(DEBWT_ENOMEM);
    for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) return fail(DEBWT_EDEVICE);
    for (auto &p : c->ev_pass) for (auto &e : p) if (hipEventCreate(&e) != hipSuccess) return fail(DEBWT_EDEVICE);
    if ((rc = ensure(c, c->rs_counts, radix_workspace_bytes(0))) != DEBWT_OK) return fail(rc);
    if ((rc = ensure(c, c->rs_over, radix_over_bytes(1 << 20))) != DEBWT_OK) return fail(rc);
    if (hipHostMalloc((void **)&c->h_over, 64, hipHostMallocDefault) != hipSuccess)
        return fail(DEBWT_ENOMEM);
    if ((rc = ensure(c, c->cp_counts, 8 * (CP_MAXCHUNKS + 16) * sizeof(u32))) != DEBWT_OK) return fail(rc);
    if ((rc = ensure(c, c->dollar, 64)) != DEBWT_OK) return fail(rc);
    *out = c;
    return DEBWT_OK;
}

extern "C" void debwt_destroy(debwt_ctx *c) {
    if (!c) return;
    if (c->special_running) { c->special_thread.join(); c->special_running = false; }
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (DevBuf *b : all_buffers(c)) if (b->p) (void)hipFree(b->p);
    if (c->h_scalars) (void)hipHostFree(c->h_scalars);
    if (c->h_over) (void)hipHostFree(c->h_over);
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    for (auto &p : c->ev_pass) for (auto &e : p) if (e) (void)hipEventDestroy(e);
    if (c->ev_copy) (void)hipEventDestroy(c->ev_copy);
    if (c->ev_copy2) (void)hipEventDestroy(c->ev_copy2);
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static void join_special(debwt_ctx *c);

extern "C" int debwt_load_text(debwt_ctx *c, const uint64_t *packed, uint64_t n, const uint64_t *sep, uint64_t nrec) {
    if (!c || !packed || !sep || nrec == 0 || n < 34) return DEBWT_EINVAL;
    join_special(c);            // a special-region thread left behind by a failed stage still reads the text of the load before
    if (sep[nrec - 1] != n - 1) return DEBWT_EINVAL;
    uint64_t prev = 0;
    for (uint64_t r = 0; r < nrec; r++) {
        uint64_t start = r ? sep[r - 1] + 1 : 0;
        if (sep[r] < start + 33 || sep[r] >= n) return DEBWT_EINVAL;        // records > 32 bases
        prev = sep[r];
    }
    (void)prev;
    const int K = c->K;
    if (n <= nrec * (uint64_t)K) return DEBWT_EINVAL;
    uint64_t M = n - nrec * (uint64_t)K;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->stage = ST_EMPTY;                                  // a failed (re-)load leaves an unusable context, not a stale one
    c->h_text = packed;
    c->h_sep.assign(sep, sep + nrec);
    c->n = n; c->nrec = nrec; c->M = M; c->Mfull = M; c->Mctx = M; c->NS = nrec * (uint64_t)K;
    c->shard_rank = 0; c->shard_world = 1; c->key_lo = c->key_hi = 0; c->Mbase = 0; c->qbase = 0;
    c->exchange = false; c->shard_planned = false;
    c->ranges.clear(); c->plan_valid = false;
    size_t tw = (size_t)((n + 63) >> 5) + 2, bw = (size_t)(n >> 6) + 3;
    ENSURE(c, c->text, tw * 8);
    ENSURE(c, c->sepbits, bw * 8);
    ENSURE(c, c->sep, nrec * 8);
    const size_t words = (size_t)((n + 63) >> 5);
    DrainOnError drain{c};                                 // from here on `packed` and `sep` are being read by queued copies
    HIPCHK(c, hipMemcpyAsync(c->sep.p, sep, nrec * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->sepbits.p, 0, bw * 8, c->stream));
    k_set_sepbits<<<grid_for(nrec, 256), 256, 0, c->stream>>>(c->sep.as<u64>(), nrec, c->sepbits.as<u64>());
    HIPCHK(c, hipMemsetAsync(c->text.as<u64>() + words, 0, (tw - words) * 8, c->stream));
    c->census_valid = false;
    if (n >= (1ull << 31)) {
        // A text of this size will be built in key ranges, cut on the census of its 12-mer prefixes (plan_ranges): the text
        // travels in pieces on a second stream and the census of a piece runs while the next one is on its way (8 ms at
        // 30 Gbp that no longer stand between the load and the first key range).
        if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        if (!c->ev_copy) HIPCHK(c, hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming));
        if (!c->ev_copy2) HIPCHK(c, hipEventCreateWithFlags(&c->ev_copy2, hipEventDisableTiming));
        ENSURE(c, c->shard_hist, SHARD_BINS * 8);
        HIPCHK(c, hipMemsetAsync(c->shard_hist.p, 0, SHARD_BINS * 8, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_copy, c->stream));                       // the separator bitmap and the zeroed census
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0));            // (the buffers may still be in use by the load before)
        const size_t piece = (size_t)1 << 24;                                   // 128 MB = 2^29 positions
        const size_t npieces = (words + piece - 1) / piece;
        for (size_t k = 0; k <= npieces; k++) {
            if (k < npieces) {
                const size_t a = k * piece, b = std::min(words, a + piece);
                HIPCHK(c, hipMemcpyAsync(c->text.as<u64>() + a, packed + a, (b - a) * 8, hipMemcpyHostToDevice, c->copy_stream));
                HIPCHK(c, hipEventRecord((k & 1) ? c->ev_copy2 : c->ev_copy, c->copy_stream));
                HIPCHK(c, hipStreamWaitEvent(c->stream, (k & 1) ? c->ev_copy2 : c->ev_copy, 0));
            }
            if (k >= 1) {                                                       // census of piece k - 1: its last word needs piece k's first
                const u64 p0 = (u64)(k - 1) * piece * 32, p1 = std::min<u64>(n, (u64)k * piece * 32);
                if (p1 > p0)
                    k_prefix_hist_words<<<1024, DEBWT_BLOCK, 0, c->stream>>>(c->text.as<u64>(), c->sepbits.as<u64>(), p0, p1, c->K,
                                                                              c->shard_hist.as<u64>());
            }
        }
        c->census.resize(SHARD_BINS);
        HIPCHK(c, hipMemcpyAsync(c->census.data(), c->shard_hist.p, SHARD_BINS * 8, hipMemcpyDeviceToHost, c->stream));
        c->census_valid = true;                                                 // (once the stream has drained, below)
    } else {
        HIPCHK(c, hipMemcpyAsync(c->text.p, packed, words * 8, hipMemcpyHostToDevice, c->stream));
    }
    // workspace that depends only on n (the key buffers are sized per key range in debwt_kmer_sort_rle)
    ENSURE(c, c->head_keys, nrec * 8);
    ENSURE(c, c->spkey, c->NS * 8);
    ENSURE(c, c->sprow, c->NS * 8);
    ENSURE(c, c->spchr, c->NS + 64);
    ENSURE(c, c->bwt, (size_t)((n + 31) >> 5) * 8 + 64);
    ENSURE(c, c->hmask, (size_t)((n + 31) >> 5) * 4 + 64);
    ENSURE(c, c->hash_rows, nrec * 8 + 64);
    int rc = sync_check(c);
    if (rc) return rc;
    drain.armed = false;                                   // (both streams have drained: the text copies are ordered before c->stream)
    c->stage = ST_LOADED;
    memset(&c->st, 0, sizeof c->st);
    c->st.n = n; c->st.nrec = nrec; c->st.n_main = M;
    return DEBWT_OK;
}

static_assert(sizeof(debwt_packed_text) == sizeof(PackedText), "C ABI mirror of PackedText");

extern "C" int debwt_pack_fasta_opts(const char *path, int threads, unsigned flags, uint64_t seed, debwt_packed_text *out,
                                     char *errbuf, size_t errlen) {
    if (!path || !out || (flags & ~DEBWT_FASTA_IUPAC_RANDOM)) return DEBWT_EINVAL;
    memset(out, 0, sizeof *out);
    return pack_fasta_file(path, threads, reinterpret_cast<PackedText *>(out), errbuf, errlen, IngestOpts{flags, seed})
               ? DEBWT_EINVAL : DEBWT_OK;
}
extern "C" int debwt_pack_fasta(const char *path, int threads, debwt_packed_text *out, char *errbuf, size_t errlen) {
    return debwt_pack_fasta_opts(path, threads, 0, 0, out, errbuf, errlen);
}
extern "C" void debwt_free_packed(debwt_packed_text *p) { free_packed_text(reinterpret_cast<PackedText *>(p)); }
extern "C" uint64_t debwt_fasta_text_bound(const char *path) { return path ? fasta_text_bound(path) : 0; }
extern "C" void debwt_host_release_hold(int on) { release_hold(on); }

extern "C" int debwt_load_fasta_opts(debwt_ctx *c, const char *path, int threads, unsigned flags, uint64_t seed) {
    if (!c || !path || (flags & ~DEBWT_FASTA_IUPAC_RANDOM)) return DEBWT_EINVAL;
    PackedText pt{};
    char msg[256] = "";
    struct Hold { Hold() { release_hold(1); } ~Hold() { release_hold(0); } } hold;      // (the ingest's buffers are released behind the load)
    if (pack_fasta_file(path, threads, &pt, msg, sizeof msg, IngestOpts{flags, seed})) { c->err = msg; return DEBWT_EINVAL; }
    c->own_text.assign(pt.words, pt.words + pt.nwords);
    std::vector<uint64_t> sep(pt.sep, pt.sep + pt.nrec);
    const uint64_t n = pt.n;
    free_packed_text(&pt);
    return debwt_load_text(c, c->own_text.data(), n, sep.data(), sep.size());
}
extern "C" int debwt_load_fasta(debwt_ctx *c, const char *path, int threads) {
    return debwt_load_fasta_opts(c, path, threads, 0, 0);
}

extern "C" int debwt_set_range_cap(debwt_ctx *c, uint64_t max_instances) {
    if (!c || max_instances < 4096) return DEBWT_EINVAL;
    c->range_cap = std::min<uint64_t>(max_instances, 0xFFFFFFF0ull - 1);
    c->plan_valid = false;
    return DEBWT_OK;
}

extern "C" int debwt_load_ascii(debwt_ctx *c, const char *seq, const uint64_t *reclen, uint64_t nrec) {
    if (!c || !seq || !reclen || !nrec) return DEBWT_EINVAL;
    uint64_t n = nrec;
    for (uint64_t r = 0; r < nrec; r++) {
        if (reclen[r] <= 32) return DEBWT_EINVAL;                              // src/collect#$.c:41-45
        n += reclen[r];
    }
    std::vector<uint64_t> words(((n + 63) >> 5) + 2, 0), sep(nrec);
    uint64_t o = 0, s = 0;
    auto put = [&](uint64_t j, uint64_t code) { words[j >> 5] |= code << ((31 - (j & 31)) << 1); };
    for (uint64_t r = 0; r < nrec; r++) {
        for (uint64_t j = 0; j < reclen[r]; j++, s++, o++) {
            uint64_t code;
            switch (seq[s]) {                                                  // src/main.c:18-23
                case 'A': case 'a': code = 0; break;
                case 'C': case 'c': code = 1; break;
                case 'G': case 'g': code = 2; break;
                case 'T': case 't': code = 3; break;
                default: return DEBWT_EINVAL;
            }
            put(o, code);
        }
        put(o, 3); sep[r] = o; o++;                                            // 'T' at the separator
    }
    for (uint64_t j = 0; j < 32; j++) put(o + j, 3);                           // src/collect#$.c:87-90
    c->own_text.swap(words);
    return debwt_load_text(c, c->own_text.data(), n, sep.data(), nrec);
}

// ---------------------------------------------------------------------------------------------------
// stage 1: keys, sort, RLE                                                            (a-1, a-2, a-3)

// Largest number of node instances one key range may hold: what the free HBM allows at `per_key` bytes of range
// workspace (key buffers, distinct keys, first instances, classification bytes; in exchange mode also the caller's
// send buffer) next to `later` bytes the later stages hold, and always below 2^32 (per-range indices are 32-bit).
static int default_range_cap(debwt_ctx *c, u64 per_key, u64 later, u64 caller_held, u64 *cap) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    u64 held = caller_held;                                  // what this build reuses: the context's own buffers and the
    for (DevBuf *b : all_buffers(c)) held += b->cap;         // caller's exchange buffers -- the plan of a repeated build
    const u64 avail = (free_b + held) / 100 * 94;            // equals the first; 6 %: allocator granularity, RCCL, runtime
    u64 rc = avail > later + (per_key << 28) ? (avail - later) / per_key : (1ull << 28);
    *cap = std::min<u64>(rc, 0xFFFFFFF0ull - (1ull << 20));
    return DEBWT_OK;
}

// Cuts the prefix bins [bin_lo, bin_hi) of the census `hist` into key ranges of at most `cap` node instances each
// (near-equal ranges; the reference balances its sort threads on the same census, src/mySort.c:98-110).
// Key bounds of the prefix bins [lo, hi) at kb key bits (key_hi = 0: no upper bound).  A shard without bins needs bounds that
// say so: [4096, 4096) -- a shard whose splitter target lies inside the last bin starts behind it -- has no first key (at
// kb = 64 the shift wraps to 0), and [0, 0) -- more shards than keys -- has no last one; with key_lo = key_hi = 0 both read
// "the whole key space": every key of the text scattered into the key buffer of a shard of 0 keys, every special suffix
// claimed by it.  They are the empty range at the nearest bin bound that a key can stand for, like any other empty shard.
static void bin_range_keys(u32 lo, u32 hi, int kb, u64 *key_lo, u64 *key_hi) {
    if (lo >= hi) { *key_lo = *key_hi = (u64)std::min<u32>(std::max<u32>(lo, 1u), SHARD_BINS - 1) << (kb - 12); return; }
    *key_lo = (u64)lo << (kb - 12);
    *key_hi = hi == SHARD_BINS ? 0ull : ((u64)hi << (kb - 12));
}

static int cut_ranges(debwt_ctx *c, const u64 *hist, u32 bin_lo, u32 bin_hi, u64 cap, u64 Mshard) {
    c->ranges.clear();
    cap = std::min<u64>(cap, 0xFFFFFFF0ull - 1);
    const u64 P = std::max<u64>(1, (Mshard + cap - 1) / cap);
    const u64 per = (Mshard + P - 1) / P;
    const u64 limit = std::min(cap, per + per / 16);            // near-equal ranges, never above the cap
    const int kb = 2 * c->cfg.k;
    auto push = [&](u32 lo, u32 hi, u64 m, u64 base) {
        debwt_ctx::KeyRange q{};
        bin_range_keys(lo, hi, kb, &q.key_lo, &q.key_hi);
        q.M = m; q.Mbase = base;
        c->ranges.push_back(q);
    };
    u64 acc = 0, base = 0, total = 0;
    u32 lo = bin_lo;
    for (u32 b = bin_lo; b < bin_hi; b++) {
        // a bin above the cap becomes a range of its own (the cap is a target; 2^32 instances is the hard limit)
        if (hist[b] >= 0xFFFFFFF0ull - (1ull << 20)) { c->err = "one 12-mer prefix bin holds 2^32 node instances or more"; return DEBWT_ERANGE; }
        if (acc && acc + hist[b] > limit) { push(lo, b, acc, base); base += acc; acc = 0; lo = b; }
        acc += hist[b]; total += hist[b];
    }
    push(lo, bin_hi, acc, base);
    if (total != Mshard) { c->err = "prefix census differs from the number of node instances"; return DEBWT_EINTERNAL; }
    return DEBWT_OK;
}

// The key ranges of this build.  One GPU: the whole key space, cut by the census of the text when it exceeds the range
// cap.  A shard: the ranges debwt_shard_plan cut, or the one range debwt_shard_set_range gave.
static int plan_ranges(debwt_ctx *c) {
    c->local_done = false;
    if (c->shard_world == 1 && !c->shard_planned) { c->key_lo = c->key_hi = 0; c->Mctx = c->Mfull; c->Mbase = 0; c->exchange = false; }
    if (c->shard_planned || (c->plan_valid && c->ranges.size() > 1 && c->shard_world == 1)) {
        // cut by debwt_shard_plan / by the census an earlier build of this text took: same cuts
        for (auto &r : c->ranges) { r.Q = r.qbase = r.B = r.Bbase = r.s0 = r.s1 = r.l0 = r.nl = 0; }
        return DEBWT_OK;
    }
    c->ranges.clear();
    u64 range_cap = c->range_cap;
    if (!range_cap) {
        // ~30 bytes per key of range workspace next to what the later stages hold for the whole text
        // (~4 bytes per position: row symbols, SP code, flag masks, blue entries, BWT)
        int rc = default_range_cap(c, 30, 4 * c->n + (8ull << 30), 0, &range_cap);
        if (rc) return rc;
        if (range_cap >= c->Mfull && c->Mfull < 0xFFFFFFF0ull) range_cap = c->Mfull;
    }
    if (c->shard_world > 1 || c->Mfull <= range_cap) {
        if (c->Mctx >= 0xFFFFFFF0ull) { c->err = "a key range must hold fewer than 2^32 node instances"; return DEBWT_ERANGE; }
        debwt_ctx::KeyRange r{};
        r.key_lo = c->key_lo; r.key_hi = c->key_hi; r.M = c->Mctx;
        c->ranges.push_back(r);
        return DEBWT_OK;
    }
    std::vector<u64> hist(SHARD_BINS);
    int rc;
    if (c->census_valid) hist = c->census;                      // taken behind the upload of the text (debwt_load_text)
    else {
        ENSURE(c, c->shard_hist, SHARD_BINS * 8);
        HIPCHK(c, hipMemsetAsync(c->shard_hist.p, 0, SHARD_BINS * 8, c->stream));
        k_prefix_hist_words<<<2048, DEBWT_BLOCK, 0, c->stream>>>(c->text.as<u64>(), c->sepbits.as<u64>(), 0, c->n, c->K,
                                                                  c->shard_hist.as<u64>());
        HIPCHK(c, hipMemcpyAsync(hist.data(), c->shard_hist.p, SHARD_BINS * 8, hipMemcpyDeviceToHost, c->stream));
        if ((rc = sync_check(c))) return rc;
    }
    if ((rc = cut_ranges(c, hist.data(), 0, SHARD_BINS, range_cap, c->Mfull))) return rc;
    c->plan_valid = true;
    return DEBWT_OK;
}

static int classify_local(debwt_ctx *c);
static int append_range(debwt_ctx *c, debwt_ctx::KeyRange &r);

static void join_special(debwt_ctx *c) {
    if (c->special_running) { c->special_thread.join(); c->special_running = false; }
}

// ---- special-region module on the device (special_kernels.h) --------------------------------------------

static int bits_for(u64 v) { int b = 1; while (b < 64 && (v >> b)) b++; return b; }     // bits that hold 0..v

// Collections of many records build their special-region tables on the device: from 2^14 special suffixes on
// (DEBWT_SPECIAL_DEVICE_MIN overrides; tests force either path), as long as the payload fields of its sorts hold the
// record ranks and item places (2^27 records, 2^32 special suffixes -- beyond that the host threads take over).
static bool special_wants_device(debwt_ctx *c) {
    const char *e = getenv("DEBWT_SPECIAL_DEVICE_MIN");
    const u64 dev_min = e ? strtoull(e, nullptr, 10) : (1ull << 14);
    if (c->NS < dev_min) return false;
    if (!(c->nrec < (1ull << 27) && c->NS < (1ull << 32) && 5 + bits_for(c->nrec) + bits_for(c->NS - 1) <= 64)) return false;
    // its workspace (59 bytes per special suffix + 12 for their positions, ~60 per record) must fit beside what the build
    // holds by now -- else the host threads build the tables, as for any collection before round 3
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    if (const char *f = getenv("DEBWT_SPECIAL_FAKE_FREE_BYTES")) free_b = (size_t)strtoull(f, nullptr, 10);   // tests: this branch
    const u64 need = c->NS * 72 + c->nrec * 64 + (64ull << 20);
    const u64 have = free_b + c->sx.cap + c->sppos.cap + c->sprec.cap + c->tail_d.cap;
    return need + (have >> 4) < have;                          // and 1/16 of it stays free
}

// the branch list (c->branch, c->nbranch) as a bitmap for the SP flags pass, where the special suffixes are many
static int special_branch_bitmap(debwt_ctx *c) {
    c->branch_bitmap = c->nbranch > 0 && c->NS >= (1ull << 14);
    if (!c->branch_bitmap) return DEBWT_OK;
    const size_t bw = (size_t)(c->n >> 6) + 3;
    ENSURE(c, c->brbits, bw * 8);
    HIPCHK(c, hipMemsetAsync(c->brbits.p, 0, bw * 8, c->stream));
    k_set_sepbits<<<grid_for(c->nbranch, 256), 256, 0, c->stream>>>(c->branch.as<u64>(), c->nbranch, c->brbits.as<u64>());
    return DEBWT_OK;
}

static int special_device_build(debwt_ctx *c, bool release_arena = true) {
    const u64 N = c->nrec, NS = c->NS, n = c->n;
    const int K = c->K;
    int rc;
    const auto t_begin = std::chrono::steady_clock::now();
    // one scratch arena, carved: u64 sort buffers of NS words, per-record and per-item side arrays
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    const size_t oX = take(NS * 8 + 64), oY = take(NS * 8 + 64);
    const size_t o_ord = take(N * 4), o_gid = take(N * 4), o_actA = take(N * 4), o_actB = take(N * 4), o_val = take(N * 8);
    const size_t o_recs = take(N * 4), o_vals = take(N * 8), o_gids = take(N * 4), o_ordv = take(N * 4);
    const size_t o_head = take((N + 1) * 4), o_stay = take(N), o_rank = take(N * 4), o_dep = take(N * 4), o_gmin = take(N * 4);
    const size_t o_grp = take(NS * 4), o_gflag = take(NS), o_headf = take(NS), o_spd = take(NS), o_item = take(NS * 16), o_bnd = take(64);
    ENSURE(c, c->sx, off);
    ENSURE(c, c->sppos, NS * 8 + 64);
    ENSURE(c, c->sprec, NS * 4 + 64);
    ENSURE(c, c->tail_d, N * 8 + 64);
    ENSURE(c, c->rs_skew, (NS / 2048 + 2) * 4);
    u8 *base = c->sx.as<u8>();
    u64 *X = (u64 *)(base + oX), *Y = (u64 *)(base + oY);
    u32 *ord = (u32 *)(base + o_ord), *gid = (u32 *)(base + o_gid), *act = (u32 *)(base + o_actA), *act2 = (u32 *)(base + o_actB);
    u64 *valbuf = (u64 *)(base + o_val), *val_s = (u64 *)(base + o_vals);
    u32 *rec_s = (u32 *)(base + o_recs), *gid_s = (u32 *)(base + o_gids), *ordv = (u32 *)(base + o_ordv);
    u32 *headpos = (u32 *)(base + o_head), *rank = (u32 *)(base + o_rank), *dep = (u32 *)(base + o_dep), *gmin = (u32 *)(base + o_gmin);
    u8 *stay = base + o_stay;
    u32 *grp = (u32 *)(base + o_grp);
    u8 *gflag = base + o_gflag, *headf = base + o_headf, *spd = base + o_spd;
    ulonglong2 *item = (ulonglong2 *)(base + o_item);
    const SxText T{c->text.as<u64>(), c->sepbits.as<u64>(), c->sep.as<u64>(), n, N, K};
    auto grid = [](u64 m) { return grid_for(m, 256); };
    auto other = [&](u64 *p_) { return p_ == X ? Y : X; };
    // stable 8-bit passes over the bits [lo, hi) of `count` words in a (scratch b); the buffer that holds the result
    auto lsd = [&](u64 *a, u64 *b, u64 count, int lo, int hi) -> u64 * {
        hipError_t e = hipSuccess;
        u64 *res = radix_sort_bits(c->stream, a, b, count, lo, hi, radix_ws(c), &e);
        if (e != hipSuccess) { c->err = std::string("special-region sort: ") + hipGetErrorString(e); return nullptr; }
        return res;
    };

    // 1. ranks of the record starts: refinement rounds on 21-symbol windows inside the tie groups
    k_sx_init<<<grid(N), 256, 0, c->stream>>>(ord, gid, act, N);
    const char *env_rounds = getenv("DEBWT_SPECIAL_MAX_ROUNDS");
    const u64 max_rounds = env_rounds ? strtoull(env_rounds, nullptr, 10) : 64ull;
    u64 na = N > 1 ? N : 0;
    bool one_group = true;
    const bool host_ties = getenv("DEBWT_SPECIAL_HOST_TIES") != nullptr;     // tests, A/B: the long-tied groups by host comparison
    bool jumping = false;
    for (u64 w = 0; na; w++) {
        if (w >= max_rounds && host_ties) {
            // records identical for max_rounds * 21 symbols and more: the few groups left are ordered on the host
            std::vector<u32> h_ord(N), h_gid(N), h_act(na);
            HIPCHK(c, hipMemcpyAsync(h_ord.data(), ord, N * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_gid.data(), gid, N * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_act.data(), act, na * 4, hipMemcpyDeviceToHost, c->stream));
            if ((rc = sync_check(c))) return rc;
            special_order_record_starts(c->h_text, n, c->h_sep.data(), N, h_ord.data(), h_gid.data(), h_act.data(), na);
            HIPCHK(c, hipMemcpyAsync(ord, h_ord.data(), N * 4, hipMemcpyHostToDevice, c->stream));
            if ((rc = sync_check(c))) return rc;
            break;
        }
        if (w >= max_rounds) {
            // ... on the device: jump rounds (special_kernels.h) -- every group's depth advances by the windows all its members
            // share with its head, then the window round below tells at least one member apart
            if (!jumping) { k_sx_depth_init<<<grid(na), 256, 0, c->stream>>>(act, na, (u32)w, dep); jumping = true; }
            HIPCHK(c, hipMemsetAsync(gmin, 0xFF, N * 4, c->stream));
            k_sx_lcp_min<<<grid(na * 64), 256, 0, c->stream>>>(T, ord, gid, act, na, dep, gmin);
            k_sx_depth_add<<<grid(na), 256, 0, c->stream>>>(gid, act, na, gmin, dep, 0u);
        }
        const int bA = bits_for(na - 1);
        k_sx_round_keys<<<grid(na), 256, 0, c->stream>>>(T, ord, act, na, w, bA, valbuf, X, jumping ? dep : nullptr);
        // three stable sorts, least significant field first: low 32 bits of the window, its high 31 bits, the tie group
        u64 *r = lsd(X, Y, na, bA, bA + 32);
        if (!r) return DEBWT_EDEVICE;
        u64 *o = other(r);
        k_sx_rekey<<<grid(na), 256, 0, c->stream>>>(r, valbuf, gid, act, na, bA, 0, o);
        if (!(r = lsd(o, other(o), na, bA, bA + 31))) return DEBWT_EDEVICE;
        if (!one_group) {
            o = other(r);
            k_sx_rekey<<<grid(na), 256, 0, c->stream>>>(r, valbuf, gid, act, na, bA, 1, o);
            if (!(r = lsd(o, other(o), na, bA, bA + bits_for(N - 1)))) return DEBWT_EDEVICE;
        }
        k_sx_gather<<<grid(na), 256, 0, c->stream>>>(r, bA, valbuf, ord, gid, act, na, rec_s, val_s, gid_s);
        SxHeadF fh{gid_s, val_s, ordv, headpos};
        if ((rc = cp_count(c, fh, na, cp_area(c, 0), 20))) return rc;
        if ((rc = cp_emit(c, fh, na, cp_area(c, 0)))) return rc;
        k_sx_sentinel<<<1, 1, 0, c->stream>>>(headpos, cp_area(c, 0) + CP_MAXCHUNKS, (u32)na);
        k_sx_apply<<<grid(na), 256, 0, c->stream>>>(rec_s, ordv, headpos, act, na, ord, gid, stay);
        SxStayF fs{stay, act, act2};
        if ((rc = cp_count(c, fs, na, cp_area(c, 1), 21))) return rc;
        if ((rc = cp_emit(c, fs, na, cp_area(c, 1)))) return rc;
        if ((rc = sync_check(c))) return rc;
        na = c->h_scalars[21];
        std::swap(act, act2);
        one_group = false;
        if (jumping && na) k_sx_depth_add<<<grid(na), 256, 0, c->stream>>>(gid, act, na, nullptr, dep, 1u);   // the window just used
    }
    k_sx_rank_of<<<grid(N), 256, 0, c->stream>>>(ord, N, rank);

    // 2. the N*K special suffixes by (key, later separator first, follower rank): three stable passes, least significant first
    const int bR = bits_for(N), bP = bits_for(NS - 1);
    u64 *r = nullptr;
    (void)o_bnd;
    k_it_pass1<<<grid(NS), 256, 0, c->stream>>>(T, rank, NS, bR, bP, X, item);
    if (!(r = lsd(X, Y, NS, bP, bP + 5 + bR))) return DEBWT_EDEVICE;
    for (int hi = 0; hi < 2; hi++) {
        u64 *o = other(r);
        k_it_rekey<<<grid(NS), 256, 0, c->stream>>>(item, r, NS, hi, bP, o);
        if (!(r = lsd(o, other(o), NS, bP, bP + 31))) return DEBWT_EDEVICE;
    }
    k_it_out<<<grid(NS), 256, 0, c->stream>>>(T, item, r, bP, NS, c->spkey.as<u64>(), c->spchr.as<u8>(), c->sppos.as<u64>(),
                                              c->sprec.as<u32>(), spd);

    // 3. special branches; head and tail nodes
    SxBranchF fb{T, c->sppos.as<u64>(), c->sprec.as<u32>(), c->spkey.as<u64>(), spd, headf, grp};
    if ((rc = cp_count(c, fb, NS, cp_area(c, 0), 20))) return rc;
    if ((rc = cp_emit(c, fb, NS, cp_area(c, 0)))) return rc;
    HIPCHK(c, hipMemsetAsync(gflag, 0, NS, c->stream));
    k_br_diff<<<grid(NS), 256, 0, c->stream>>>(T, c->sppos.as<u64>(), grp, NS, gflag);
    SxBranchEmitF fe{gflag, grp, c->sppos.as<u64>(), nullptr};
    if ((rc = cp_count(c, fe, NS, cp_area(c, 1), 21))) return rc;
    if ((rc = sync_check(c))) return rc;
    c->nbranch = c->h_scalars[21];
    ENSURE(c, c->branch, c->nbranch * 8 + 64);
    if (c->nbranch) {
        fe.branch = X;
        if ((rc = cp_emit(c, fe, NS, cp_area(c, 1)))) return rc;
        if (!(r = lsd(X, Y, c->nbranch, 0, bits_for(n)))) return DEBWT_EDEVICE;
        HIPCHK(c, hipMemcpyAsync(c->branch.p, r, c->nbranch * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    k_heads_tails<<<grid(N), 256, 0, c->stream>>>(T, X, c->tail_d.as<u64>());
    if (!(r = lsd(X, Y, N, 0, 2 * K + 2))) return DEBWT_EDEVICE;
    HIPCHK(c, hipMemcpyAsync(c->head_keys.p, r, N * 8, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = special_branch_bitmap(c))) return rc;
    if ((rc = sync_check(c))) return rc;
    if (release_arena) {
        // The arena (59 bytes per special suffix) and the positions / records of the sorted items have done their work: a
        // read set whose module workspace is a large share of the HBM gives it back before the key ranges and the later
        // stages allocate theirs (they have no host path to fall back to); small arenas stay for the next build.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (c->sx.cap + c->sppos.cap + c->sprec.cap) > total_b / 16)
            for (DevBuf *b : {&c->sx, &c->sppos, &c->sprec}) { HIPCHK(c, hipFree(b->p)); b->p = nullptr; b->cap = 0; }
    }
    c->special_dev = true;
    c->st.ms_host_special = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    c->st.special_path = 2;
    c->st.special_threads = 0;
    return DEBWT_OK;
}

// how the key sort of a range divides its key bits (what sort_range's radix_sort_u64 will decide)
static RadixSplit range_split(const debwt_ctx *c, const debwt_ctx::KeyRange &r) {
    const u64 range[2] = {r.key_lo, r.key_hi};
    return radix_split(r.M, 2 * c->cfg.k, c->cfg.sort_algo, range, r.heavy);
}

// Sampled census of the 12-mer prefixes (the top 24 key bits) of the text's nodes: one position in HEAVY_STRIDE (a prime:
// no beat with tandem repeats) adds to one of 2^24 counters; k_heavy_bins then sums, per 12-bit bin of the range planner,
// the counters above `limit` samples and keeps the largest.  The bucket pass gives a 12-mer bin to ONE workgroup, which
// takes a bin above RS_BUCKET_HEAVY keys in two reads of global memory at a few per cent of the rate of the rest.
#define HEAVY_STRIDE 251u
__global__ __launch_bounds__(256) void k_prefix24_sample(const u64 *__restrict__ text, const u64 *__restrict__ sepbits, u64 n, int K,
                                                         u32 *__restrict__ bins) {
    const u64 kmask = K >= 64 ? ~0ull : (1ull << K) - 1ull;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j * HEAVY_STRIDE + (u64)K <= n; j += (u64)gridDim.x * blockDim.x) {
        const u64 pos = j * HEAVY_STRIDE;
        if (sep_window(sepbits, pos) & kmask) continue;               // no node starts here
        atomicAdd(&bins[(u32)(text_window(text, pos) >> 40)], 1u);
    }
}
__global__ __launch_bounds__(256) void k_heavy_bins(const u32 *__restrict__ bins, u32 limit, u64 *__restrict__ sum, u32 *__restrict__ top) {
    for (u32 b = blockIdx.x * blockDim.x + threadIdx.x; b < (1u << 24); b += gridDim.x * blockDim.x) {
        const u32 v = bins[b];
        if (v > limit) { atomicAdd(&sum[b >> 12], (u64)v); atomicMax(&top[b >> 12], v); }
    }
}

// Which key ranges leave the bucket pass alone (KeyRange::heavy): those where more than 1/64 of the keys sit in 12-mer bins
// above RS_BUCKET_HEAVY keys, or one bin holds four times that (distribution R: Alu-like 12-mers with 10^7 instances).
// Only ranges that would take the bucket pass are asked, once per plan; the counters borrow key buffer B.
static int heavy_ranges(debwt_ctx *c) {
    const int kb = 2 * c->cfg.k;
    bool ask = false;
    for (auto &r : c->ranges) {
        const u64 range[2] = {r.key_lo, r.key_hi};
        if (!r.heavy_known && radix_split(r.M, kb, c->cfg.sort_algo, range, false).bucket) ask = true;
    }
    const size_t need = ((size_t)4 << 24) + SHARD_BINS * 12;
    if (!ask || c->K < 12 || kb < 24 || c->keysB.cap < need || c->n < (u64)c->K) return DEBWT_OK;
    u32 *bins = c->keysB.as<u32>();
    u64 *d_sum = reinterpret_cast<u64 *>(bins + (1u << 24));
    u32 *d_top = reinterpret_cast<u32 *>(d_sum + SHARD_BINS);
    HIPCHK(c, hipMemsetAsync(bins, 0, need, c->stream));
    k_prefix24_sample<<<4096, 256, 0, c->stream>>>(c->text.as<u64>(), c->sepbits.as<u64>(), c->n, c->K, bins);
    k_heavy_bins<<<4096, 256, 0, c->stream>>>(bins, RS_BUCKET_HEAVY / HEAVY_STRIDE, d_sum, d_top);
    std::vector<u64> sum(SHARD_BINS);
    std::vector<u32> top(SHARD_BINS);
    HIPCHK(c, hipMemcpyAsync(sum.data(), d_sum, SHARD_BINS * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(top.data(), d_top, SHARD_BINS * 4, hipMemcpyDeviceToHost, c->stream));
    int rc = sync_check(c);
    if (rc) return rc;
    for (auto &r : c->ranges) {
        const u32 lo = (u32)(r.key_lo >> (kb - 12)), hi = r.key_hi ? (u32)(r.key_hi >> (kb - 12)) : SHARD_BINS;
        u64 in_heavy = 0, largest = 0;
        for (u32 b = lo; b < hi; b++) { in_heavy += sum[b] * HEAVY_STRIDE; largest = std::max<u64>(largest, (u64)top[b] * HEAVY_STRIDE); }
        r.heavy = in_heavy > r.M / 64 || largest > 4ull * RS_BUCKET_HEAVY;
        r.heavy_known = true;
        if (getenv("DEBWT_TRACE_SORT"))
            fprintf(stderr, "key range [%u, %u) of %llu keys: ~%llu in 12-mer bins above %u keys, the largest ~%llu: %s\n", lo, hi,
                    (unsigned long long)r.M, (unsigned long long)in_heavy, (unsigned)RS_BUCKET_HEAVY, (unsigned long long)largest,
                    r.heavy ? "four HBM passes" : "bucket pass");
    }
    return DEBWT_OK;
}

// plans the ranges, sizes the range workspace, starts the host special-region module
static int sort_begin(debwt_ctx *c) {
    const u64 n = c->n;
    if (c->stage > ST_LOADED) c->stage = ST_LOADED;       // a new build: what the stages of the last one left is scratch (reclaim)
    int rc = plan_ranges(c);
    if (rc) return rc;
    u64 maxM = 0;
    for (auto &r : c->ranges) maxM = std::max(maxM, r.M);
    struct ReclaimScope { debwt_ctx *c; ~ReclaimScope() { c->reclaim_ok = false; } } rscope{c};
    c->reclaim_ok = true;                                 // (nothing of the last build's SP stage and blue sort is needed again)
    if (!c->exchange) ENSURE(c, c->keysA, maxM * 8 + 64);          // exchange mode: the received keys are buffer A
    ENSURE(c, c->keysB, maxM * 8 + 64);
    ENSURE(c, c->rs_skew, (maxM / 2048 + 2) * 4);
    ENSURE(c, c->rs_rle, radix_rle_ws_bytes(maxM));
    if ((rc = heavy_ranges(c))) return rc;
    size_t pair_bytes = 0;                                // the joint counts of every range fit what the widest one needs
    for (auto &r : c->ranges) {
        const u64 range[2] = {r.key_lo, r.key_hi};
        pair_bytes = std::max(pair_bytes, radix_pair_bytes_u64(r.M, 2 * c->cfg.k, range, r.heavy));
    }
    ENSURE(c, c->rs_pair, pair_bytes);
    ENSURE(c, c->dk, maxM * 8 + 64);
    ENSURE(c, c->dstart, maxM * 4 + 64);
    ENSURE(c, c->pflag, maxM + 64);                      // classification byte per distinct key of a range
    ENSURE(c, c->mchar, c->Mctx + 64);
    c->reclaim_ok = false;
    c->Q = c->B = c->nlarge = 0; c->nfacts_acc = 0; c->n1024 = 0; c->n512 = 0; c->Dsum = 0;
    c->st.sort_unfit_stretches = c->st.sort_unfit_network = c->st.sort_over_stretches = c->st.sort_bucket_passes = 0;
    const size_t P = c->ranges.size();
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    // the keys (node << 2 | pred) are read off the text inside the first radix pass: no unsorted key array
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    // special-region module (src/collect#$.c:118-157,348-602): on the device for collections of many records, else on the
    // host beside the GPU's key sort
    join_special(c);
    c->special_dev = false;
    if (special_wants_device(c)) {
        if ((rc = special_device_build(c))) return rc;
    } else {
    c->special_running = true;
    c->special_thread = std::thread([c, n]() {
        auto t0 = std::chrono::steady_clock::now();
        build_special_tables(c->h_text, n, c->h_sep.data(), c->nrec, c->K, &c->special);
        c->st.ms_host_special = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        c->st.special_threads = c->special.threads_used;
        c->st.special_path = c->special.threads_used > 1 ? 1 : 0;
    });
    }
    // several ranges read off the text: the chunk histograms of every range's first pass from ONE scan of the text (a
    // lane per text word, radix_text_hist_ranges); a single range of a long text takes the same kernel -- it is twice
    // as fast as the histogram pass of the sort itself (a shard of 8 reads the whole text for its one range)
    c->shared_hist = P <= RS_MAX_RANGES && !c->exchange &&
                     (P > 1 || (P == 1 && n >= (1ull << 26) && range_split(c, c->ranges[0]).hbm_shift > 0));
    if (c->shared_hist) {
        const int kb = 2 * c->cfg.k;
        std::vector<u8> rob(SHARD_BINS, 0xFF);
        int shifts[RS_MAX_RANGES];
        for (size_t i = 0; i < P; i++) {
            const u32 lo = (u32)(c->ranges[i].key_lo >> (kb - 12));
            const u32 hi = c->ranges[i].key_hi ? (u32)(c->ranges[i].key_hi >> (kb - 12)) : SHARD_BINS;
            for (u32 b = lo; b < hi; b++) rob[b] = (u8)i;
            shifts[i] = range_split(c, c->ranges[i]).hbm_shift;
        }
        ENSURE(c, c->dest_tab, SHARD_BINS);
        ENSURE(c, c->range_hist, P * radix_text_hist_stride() * sizeof(u32));
        HIPCHK(c, hipMemcpyAsync(c->dest_tab.p, rob.data(), SHARD_BINS, hipMemcpyHostToDevice, c->stream));
        TextKeySrc all{c->text.as<u64>(), c->sepbits.as<u64>(), n, c->K, 0, 0, 0, nullptr, nullptr, 0};
        hipError_t e = radix_text_hist_ranges(c->stream, all, c->dest_tab.as<u8>(), kb, shifts, (int)P, c->range_hist.as<u32>());
        if (e != hipSuccess) { c->err = std::string("range histograms: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
        HIPCHK(c, hipStreamSynchronize(c->stream));          // rob is host memory
    }
    return DEBWT_OK;
}

// sorts, run-length encodes and (unless it is the only range of a text-fed build) classifies range i.
// imported: the range's keys in a caller-owned DEVICE buffer (exchange mode: it serves as key buffer A and must stay
// valid until the next range or debwt_shard_sort_end), else the keys are read off the text.
static int sort_range(debwt_ctx *c, size_t i, u64 *imported) {
    const u64 n = c->n;
    const size_t P = c->ranges.size();
    debwt_ctx::KeyRange &r = c->ranges[i];
    int rc;
    c->M = r.M;
    c->sort_a = imported ? imported : c->keysA.as<u64>();
    c->sort_b = c->keysB.as<u64>();
    TextKeySrc ts{c->text.as<u64>(), c->sepbits.as<u64>(), n, c->K, r.key_lo, r.key_hi, 0,
                  c->shared_hist ? c->range_hist.as<u32>() + i * radix_text_hist_stride() : nullptr, nullptr, 0};
    // the bucket finish of the sort counts the distinct keys of its tiles and the encoding follows tile by tile
    // (tune bit 8 = 256: separate count and emit passes over the sorted keys instead)
    RleSink sink{c->dk.as<u64>(), c->dstart.as<u32>(), c->mchar.as<u8>() + r.Mbase, c->rs_rle.p, &c->h_scalars[0],
                 &c->h_scalars[32], 0, (c->cfg.reserved & 131072) != 0,           // bit 17: no staging of distinct keys
                 // the sorted keys can be asked for (debwt_fetch_array) after the sort stage of a one-range build driven
                 // stage by stage on one GPU, and by nobody else: every other build keeps the encoding only (tune bit 23: keeps both -- A/B)
                 (P > 1 || c->exchange || c->whole_build || c->shard_world > 1) && !(c->cfg.reserved & 8388608), false};
    const u64 key_range[2] = {r.key_lo, r.key_hi};        // imported keys are the range's too
    if (imported && r.M < 2) c->sk = c->sort_a;
    else if ((rc = sort_keys(c, c->sort_a, c->sort_b, r.M, 2 * c->cfg.k, &c->sk, i == 0, imported ? nullptr : &ts, true,
                             (c->cfg.reserved & 256) ? nullptr : &sink, key_range, r.heavy))) return rc;
    else if (range_split(c, r).bucket) c->st.sort_bucket_passes++;
    if (P == 1 && !c->exchange) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    if (!sink.done) {
        RleF f{c->sk, c->dk.as<u64>(), c->dstart.as<u32>(), c->mchar.as<u8>() + r.Mbase};
        if ((rc = cp_count(c, f, r.M, cp_area(c, 0), 0))) return rc;
        if ((rc = cp_emit(c, f, r.M, cp_area(c, 0)))) return rc;
    }
    if (i == 0 && !c->special_dev) {
        join_special(c);
        const SpecialTables &sp = c->special;
        c->nbranch = sp.branch.size();
        ENSURE(c, c->branch, sp.branch.size() * 8 + 64);
        HIPCHK(c, hipMemcpyAsync(c->head_keys.p, sp.head_keys.data(), c->nrec * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->spkey.p, sp.key.data(), c->NS * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->spchr.p, sp.chr.data(), c->NS, hipMemcpyHostToDevice, c->stream));
        if (!sp.branch.empty())
            HIPCHK(c, hipMemcpyAsync(c->branch.p, sp.branch.data(), sp.branch.size() * 8, hipMemcpyHostToDevice, c->stream));
        if ((rc = special_branch_bitmap(c))) return rc;
    }
    // special suffixes whose key lies in this range, and their rows among the context's instances
    u64 *d_bounds = nullptr;
    {
        const std::vector<uint64_t> &key = c->special.key;          // ascending (suffix order implies key order)
        u64 s0 = 0, s1 = c->NS;
        if ((c->shard_world > 1 || P > 1) && c->special_dev) {
            d_bounds = c->dollar.as<u64>() + 5;                       // spare words behind the '$' row and the census
            k_sp_bounds<<<1, 64, 0, c->stream>>>(c->spkey.as<u64>(), c->NS, r.key_lo >> 2, r.key_hi >> 2, d_bounds);
            HIPCHK(c, hipMemcpyAsync(&c->h_scalars[24], d_bounds, 16, hipMemcpyDeviceToHost, c->stream));
        } else if (c->shard_world > 1 || P > 1) {
            s0 = std::lower_bound(key.begin(), key.end(), r.key_lo >> 2) - key.begin();
            s1 = r.key_hi ? (u64)(std::lower_bound(key.begin(), key.end(), r.key_hi >> 2) - key.begin()) : c->NS;
        }
        r.s0 = s0; r.s1 = s1;
    }
    if ((rc = sync_check(c))) return rc;
    if (d_bounds) memcpy(&r.s0, &c->h_scalars[24], 8), memcpy(&r.s1, &c->h_scalars[26], 8);
    c->D = c->h_scalars[0];
    c->Dsum += c->D;
    if (sink.done) {
        c->st.sort_unfit_stretches += c->h_scalars[32]; c->st.sort_unfit_network += c->h_scalars[35];
        c->st.sort_over_stretches += sink.n_over;
    }
    if (r.s1 > r.s0)
        k_special_rows<<<grid_for(r.s1 - r.s0, 256), 256, 0, c->stream>>>(
            c->dk.as<u64>(), c->dstart.as<u32>(), c->D, r.M, c->spkey.as<u64>() + r.s0, r.s1 - r.s0,
            r.Mbase + (r.s0 - c->ranges[0].s0), c->sprow.as<u64>() + r.s0);
    if (P > 1 || c->exchange) {
        // the range's keys are gone after this call: classify them now
        if ((rc = classify_local(c))) return rc;
        if ((rc = append_range(c, r))) return rc;
    }
    return DEBWT_OK;
}

static int sort_end(debwt_ctx *c) {
    c->s0 = c->ranges.front().s0; c->s1 = c->ranges.back().s1;
    if (c->ranges.size() > 1 || c->exchange) {
        c->local_done = true;
        HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
        HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    }
    c->st.distinct_keys = c->Dsum;
    c->st.special_branch_num = c->nbranch;
    c->stage = ST_SORTED;
    return DEBWT_OK;
}

extern "C" int debwt_kmer_sort_rle(debwt_ctx *c) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    if (c->exchange) { c->err = "exchange-mode shard: use debwt_shard_sort_begin/_range/_end"; return DEBWT_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = sort_begin(c);
    for (size_t i = 0; !rc && i < c->ranges.size(); i++) rc = sort_range(c, i, nullptr);
    join_special(c);
    if (rc) return rc;
    return sort_end(c);
}

// ---------------------------------------------------------------------------------------------------
// stage 2: classification                                                                      (a-8)

// local half: classification of this shard's distinct keys -> its fact lists [multi-out | multi-in] and its
// block table (mi_j0, mi_freq, bstart)
static int classify_local(debwt_ctx *c) {
    const u64 M = c->M, D = c->D, nrec = c->nrec;
    int rc;
    if (c->ranges.size() == 1) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    ClassifyCommon cc{c->dk.as<u64>(), c->dstart.as<u32>(), D, M, c->head_keys.as<u64>(), nrec};
    // pflag (n bytes) is free until the SP stage: it holds the per-distinct-key classification byte
    u8 *cf = c->pflag.as<u8>();
    ClassifyFlagsF ff{cc, c->K, cf};
    {
        u32 nchunks; u64 chunk;
        plan_chunks(D, &nchunks, &chunk);
        u32 *ca = cp_area(c, 1), *cb = cp_area(c, 2);
        u32 *wl = reinterpret_cast<u32 *>(c->sk == c->sort_a ? c->sort_b : c->sort_a);   // the sort's scratch buffer: >= 8 M bytes
        u32 *wl_count = cp_area(c, 7);
        if (D) {
            k_classify_flags<<<nchunks, DEBWT_BLOCK, 0, c->stream>>>(ff, chunk, ca, cb, wl, wl_count);
            k_classify_groups<<<nchunks, DEBWT_BLOCK, 0, c->stream>>>(ff, chunk, ca, cb, wl, wl_count);
        } else { HIPCHK(c, hipMemsetAsync(ca, 0, sizeof(u32), c->stream)); HIPCHK(c, hipMemsetAsync(cb, 0, sizeof(u32), c->stream)); }
        cp_scan_kernel<<<1, 1024, 0, c->stream>>>(ca, D ? nchunks : 1, ca + CP_MAXCHUNKS);
        cp_scan_kernel<<<1, 1024, 0, c->stream>>>(cb, D ? nchunks : 1, cb + CP_MAXCHUNKS);
        HIPCHK(c, hipMemcpyAsync(&c->h_scalars[1], ca + CP_MAXCHUNKS, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&c->h_scalars[2], cb + CP_MAXCHUNKS, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = sync_check(c))) return rc;
    c->rQ = c->h_scalars[1];
    c->Rmo = c->h_scalars[2];
    const u64 Q = c->rQ, Rmo = c->Rmo;
    ENSURE(c, c->facts, (Rmo + Q) * 8 + 64);
    ENSURE(c, c->mi_j0, Q * 4 + 64);
    ENSURE(c, c->mi_freq, Q * 4 + 64);
    ENSURE(c, c->bstart, Q * 4 + 64);
    ENSURE(c, c->large_tmp, Q * 4 + 64);
    u64 *facts = c->facts.as<u64>();
    {
        const u64 nslots = Q + Rmo;
        ENSURE(c, c->fact_work, nslots * 16 + 64);
        HIPCHK(c, hipMemsetAsync(c->fact_work.p, 0, nslots * 16 + 16, c->stream));
        FactEmitArgs fa{cc, c->K, cf, facts + Rmo, c->mi_j0.as<u32>(), c->mi_freq.as<u32>(), facts,
                        c->fact_work.as<uint4>()};
        u32 nchunks; u64 chunk;
        plan_chunks(D, &nchunks, &chunk);       // same chunks as the counting sweep (multiples of 1024 keys)
        if (D) k_emit_facts<<<nchunks, DEBWT_BLOCK, 0, c->stream>>>(fa, chunk, cp_area(c, 1), cp_area(c, 2));
        if (nslots) k_eval_facts<<<grid_for(nslots, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>(fa, nslots);
    }
    BlockStartF fb{c->mi_freq.as<u32>(), c->bstart.as<u32>()};
    if ((rc = cp_count(c, fb, Q, cp_area(c, 4), 4))) return rc;
    if ((rc = cp_emit(c, fb, Q, cp_area(c, 4)))) return rc;
    LargeBlockF fl{c->mi_freq.as<u32>(), BLUE_LDS_CAP, c->large_tmp.as<u32>()};
    if ((rc = cp_count(c, fl, Q, cp_area(c, 5), 5))) return rc;
    if ((rc = cp_emit(c, fl, Q, cp_area(c, 5)))) return rc;
    {
        u32 *cnt = cp_area(c, 6) + CP_MAXCHUNKS + 8;              // two free words behind the area's scan total
        HIPCHK(c, hipMemsetAsync(cnt, 0, 8, c->stream));
        if (Q) k_count_blocks<<<std::min<u32>(grid_for(Q, 256), 512u), 256, 0, c->stream>>>(c->mi_freq.as<u32>(), Q, 512u, 1024u, cnt);
        if (Q) k_count_blocks<<<std::min<u32>(grid_for(Q, 256), 512u), 256, 0, c->stream>>>(c->mi_freq.as<u32>(), Q, 256u, 512u, cnt + 1);
        HIPCHK(c, hipMemcpyAsync(&c->h_scalars[11], cnt, 8, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = sync_check(c))) return rc;
    c->rB = c->h_scalars[4];
    c->rnlarge = c->h_scalars[5];
    c->rn1024 = c->h_scalars[11];
    c->rn512 = c->h_scalars[12];
    return DEBWT_OK;
}

// appends the range just classified (facts, block tables, large-block list) to the context-wide tables
static int append_range(debwt_ctx *c, debwt_ctx::KeyRange &r) {
    const u64 Q = c->rQ, nf = c->Rmo + Q;
    r.Q = Q; r.qbase = c->Q; r.B = c->rB; r.Bbase = c->B; r.l0 = c->nlarge; r.nl = c->rnlarge;
    ENSURE_KEEP(c, c->facts_acc, (c->nfacts_acc + nf) * 8 + 64, c->nfacts_acc * 8);
    ENSURE_KEEP(c, c->blk_j0, (c->Q + Q) * 8 + 64, c->Q * 8);
    ENSURE_KEEP(c, c->blk_freq, (c->Q + Q) * 4 + 64, c->Q * 4);
    ENSURE_KEEP(c, c->blk_start, (c->Q + Q) * 8 + 64, c->Q * 8);
    ENSURE_KEEP(c, c->large_q, (c->nlarge + c->rnlarge) * 4 + 64, c->nlarge * 4);
    if (nf) HIPCHK(c, hipMemcpyAsync(c->facts_acc.as<u64>() + c->nfacts_acc, c->facts.p, nf * 8, hipMemcpyDeviceToDevice, c->stream));
    if (Q)
        k_append_blocks<<<grid_for(Q, 256), 256, 0, c->stream>>>(c->mi_j0.as<u32>(), c->mi_freq.as<u32>(), c->bstart.as<u32>(), Q,
                                                                 r.Mbase, r.Bbase, c->blk_j0.as<u64>() + r.qbase,
                                                                 c->blk_freq.as<u32>() + r.qbase, c->blk_start.as<u64>() + r.qbase);
    if (c->rnlarge) {
        HIPCHK(c, hipMemcpyAsync(c->large_q.as<u32>() + c->nlarge, c->large_tmp.p, c->rnlarge * 4, hipMemcpyDeviceToDevice, c->stream));
        if (r.qbase)
            k_offset_u32<<<grid_for(c->rnlarge, 256), 256, 0, c->stream>>>(c->large_q.as<u32>() + c->nlarge, c->rnlarge, (u32)r.qbase);
    }
    c->nfacts_acc += nf; c->Q += Q; c->B += c->rB; c->nlarge += c->rnlarge; c->n1024 += c->rn1024; c->n512 += c->rn512;
    if (c->Q >= 0xFFFFFFF0ull) { c->err = "more than 2^32 multi-in blocks"; return DEBWT_ERANGE; }
    c->facts_ready = true;
    return sync_check(c);
}

// global half: the red table from the facts of ALL shards (d_facts: device, nfacts words, any order) plus the
// tail# facts; identical on every shard
static int classify_global(debwt_ctx *c, const u64 *d_facts, u64 nfacts, u64 qbase, u64 btotal) {
    const u64 nrec = c->nrec, Q = c->Q;
    int rc;
    const u64 nf = nfacts + nrec;
    c->nfacts = nf;
    c->qbase = qbase;
    c->Btotal = btotal;
    ENSURE(c, c->facts_all, nf * 8 + 64);
    ENSURE(c, c->facts_tmp, nf * 8 + 64);
    ENSURE(c, c->rs_skew, (nf / 2048 + 2) * 4);
    ENSURE(c, c->red, nf * 8 + 64);
    ENSURE(c, c->red_q, nf * 4 + 64);
    u64 *all = c->facts_all.as<u64>();
    if (nfacts) HIPCHK(c, hipMemcpyAsync(all, d_facts, nfacts * 8, hipMemcpyDeviceToDevice, c->stream));
    if (c->special_dev) HIPCHK(c, hipMemcpyAsync(all + nfacts, c->tail_d.p, nrec * 8, hipMemcpyDeviceToDevice, c->stream));
    else HIPCHK(c, hipMemcpyAsync(all + nfacts, c->special.tail_facts.data(), nrec * 8, hipMemcpyHostToDevice, c->stream));
    u64 *sorted_facts = nullptr;
    if ((rc = sort_keys(c, all, c->facts_tmp.as<u64>(), nf, 2 * c->cfg.k, &sorted_facts, false))) return rc;
    RedUniqueF fr{sorted_facts, nf, c->red.as<u64>()};
    if ((rc = cp_count(c, fr, nf, cp_area(c, 3), 3))) return rc;
    if ((rc = cp_emit(c, fr, nf, cp_area(c, 3)))) return rc;
    if ((rc = sync_check(c))) return rc;
    c->R = c->h_scalars[3];
    const u64 R = c->R;
    RedBlockF fq{c->red.as<u64>(), c->red_q.as<u32>()};
    if ((rc = cp_count(c, fq, R, cp_area(c, 6), 6))) return rc;
    if ((rc = cp_emit(c, fq, R, cp_area(c, 6)))) return rc;
    ENSURE(c, c->blue, c->B * 8 + 64);
    if ((rc = sync_check(c))) return rc;
    if (c->shard_world == 1 && c->h_scalars[6] != Q) {
        c->err = "multi-in count mismatch between fact list and red table";
        return DEBWT_EINTERNAL;
    }
    c->st.red_capacity = R; c->st.blue_capacity = c->B; c->st.blue_bound_num = Q; c->st.case3num = 2 * Q;
    c->st.blue_large_blocks = c->nlarge;
    c->Qtotal = c->h_scalars[6];
    c->stage = ST_CLASSIFIED;
    return DEBWT_OK;
}

extern "C" int debwt_classify(debwt_ctx *c) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_SORTED) return DEBWT_ESTATE;
    if (c->shard_world > 1) { c->err = "sharded context: use debwt_shard_classify_local/_global"; return DEBWT_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc;
    if (!c->local_done) {
        c->Q = c->B = c->nlarge = 0; c->nfacts_acc = 0; c->n1024 = 0; c->n512 = 0;      // a repeated call starts over
        if ((rc = classify_local(c))) return rc;
        if ((rc = append_range(c, c->ranges[0]))) return rc;
    }
    return classify_global(c, c->facts_acc.as<u64>(), c->nfacts_acc, 0, c->B);
}

// ---------------------------------------------------------------------------------------------------
// stage 3: SP code and blue entries                                                            (a-4)

// SP stage in three steps so that a sharded build can cut it at the exchanges:
//   sp_flags   node table + flags of the text groups [g0, g1) + their multi-out / multi-in counts
//   sp_emit    SP symbols of the slice at their global offset, work list of the slice's multi-in positions
//   sp_finish  4-bit packed SP code of the WHOLE text (after the slices' symbols were all-gathered)
// node table + prefilter from the red table; flag masks sized for the whole text
static int sp_prepare(debwt_ctx *c) {
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    // (the range workspace of the key sort is idle from here on: an allocation of this function that fails may release it)
    struct ReclaimScope { debwt_ctx *c; ~ReclaimScope() { c->reclaim_ok = false; } } rscope{c};
    c->reclaim_ok = true;
    const u64 ngroups = (c->n + 31) >> 5;
    ENSURE(c, c->momask, ngroups * 4 + 64);
    ENSURE(c, c->mimask, ngroups * 4 + 64);
    // node table: 4..8 slots per red node; prefilter: ~8 bits per red node (tuning knob: reserved = delta+8)
    // (4..8 slots per red node: at 2..4 a collection whose red nodes happened to fill the table by half -- eight genomes --
    // spent 14 % more on the SP flags than one that filled it by a quarter -- ten --: 329 -> 281 ms of SP stage for 24 Gbp;
    // ten genomes 364 -> 349, with an Alu-like family 586 -> 540, one genome 32.9 -> 28.6; 8..16 slots: 3 ms more for 30 Gbp)
    int hbits = 10;
    u64 slots_per_node = 4;
    if (const char *e = getenv("DEBWT_NODE_SLOTS")) slots_per_node = std::max<u64>(2, strtoull(e, nullptr, 10));   // A/B
    while ((1ull << hbits) < slots_per_node * c->R) hbits++;
    if (hbits > 32 && (1ull << 32) >= 2 * c->R) hbits = 32;      // (slot numbers are 32-bit: 2..4 per node where 4..8 do not fit --
                                                                 //  k = 16 on a 3.1 Gbp text: 1.07 G branching 15-mers, a 64 GB table)
    // prefilter.  K >= 24: 64-bit words chosen by the node's minimizer, ~2 red nodes per word (stage_kernels.h,
    // k_build_mzfilter) -- a lane that walks 32 consecutive positions fetches ~4 words instead of probing 32 times.
    // Smaller K (or cfg.reserved bit 11: tests): one bit per hashed node, 8 bits per red node; while the node table
    // still fits the Infinity Cache (<= 256 MB) the bitmap is held at L2 size (2 MB, down to 2..4 bits per node).
    // cfg.reserved & 15 = delta + 8 overrides the size (tuning).
    // The plain bitmap is kept for small node tables (below 2^20 slots: a few Mbp); from there on the minimizer filter
    // wins (250 Mbp: SP stage 3.16 ms against 3.41 ms).  cfg.reserved bit 12 forces it for any size (tests).
    // (nodes of 16..23 symbols take minimizers of 12 symbols: k = 17..24 -- round 6)
    c->mzfilter = c->K >= 16 && !(c->cfg.reserved & 2048) && (hbits >= 20 || (c->cfg.reserved & 4096));
    c->mzw = c->K >= 24 ? MZ_W : MZ_W_SHORT;
    c->mztable = c->mzfilter && c->K >= 24 && (c->cfg.reserved & 16384);   // cfg.reserved bit 14: node table addressed by minimizer (A/B, tests)
    int pb;
    if (c->mzfilter) {
        pb = 10;
        while ((2ull << pb) < c->R) pb++;
        if (c->cfg.reserved & 15) pb += (c->cfg.reserved & 15) - 8;
        if (pb < 10) pb = 10;
        if (pb > 30) pb = 30;
    } else {
        pb = (c->cfg.reserved & 15) ? hbits + (c->cfg.reserved & 15) - 8
                                     : (hbits <= 24 ? std::max(hbits, std::min(hbits + 3, 24)) : hbits + 3);
        if (pb < 10) pb = 10;
        if (pb > 31) pb = 31;                                     // (a 256 MB bitmap: nearly every node of so small a K branches anyway)
    }
    if (pb > 31 || hbits > 32) { c->err = "more than 2^31 branching nodes: the node table has 2^32 slots"; return DEBWT_ERANGE; }
    c->hbits = hbits; c->pbits = pb;
    // absolute 32-bit fill cursors unless the context's blue slots need more bits (cfg.reserved bit 4 forces the
    // 64-bit form: tests)
    c->abs32 = c->B < 0xFFFFFFF0ull && !(c->cfg.reserved & 16);
    size_t rb_bytes = (c->mzfilter ? ((size_t)8 << pb) : ((size_t)1 << pb) / 8) + 64, ht_slots = (size_t)1 << hbits;
    ENSURE(c, c->rbits, rb_bytes);
    ENSURE(c, c->htab, ht_slots * sizeof(HSlot));
    HIPCHK(c, hipMemsetAsync(c->rbits.p, 0, rb_bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(c->htab.p, 0, ht_slots * sizeof(HSlot), c->stream));
    if (c->R) {
        k_build_hash<<<grid_for(c->R, 256), 256, 0, c->stream>>>(c->red.as<u64>(), c->R, c->red_q.as<u32>(),
                                                                c->blk_start.as<u64>(), c->abs32 ? 1 : 0, (u32)c->qbase,
                                                                (u32)c->Q, hbits, c->htab.as<HSlot>(), c->mzfilter ? 0 : pb,
                                                                c->rbits.as<u32>(), c->mztable ? c->K : 0);
        if (c->mzfilter)
            k_build_mzfilter<<<grid_for(c->R, 256), 256, 0, c->stream>>>(c->red.as<u64>(), c->R, c->K, pb, c->rbits.as<u64>(), c->mzw);
    }
    return DEBWT_OK;
}

// SP stage of the text groups [g0, g1) (a slice of fewer than 2^32 positions: the compaction counters are 32-bit):
//   sp_flags   flags of the slice + its multi-out / multi-in counts
//   sp_emit    SP symbols of the slice at their global offset, work list of the slice's multi-in positions
//   sp_finish  packed SP code of the WHOLE text (after all slices / after the slices' symbols were all-gathered)
#define SP_SLICE_GROUPS (1ull << 26)
static SpBlockIds sp_block_ids(debwt_ctx *c) {
    if (!c->route_direct) return SpBlockIds{nullptr, nullptr, nullptr, 0};
    return SpBlockIds{c->qlist.as<u32>(), c->qwave.as<unsigned long long>(), c->qwave.as<u64>() + 1, c->gq0};
}
// room for the block ids of the multi-in positions among `groups` text groups that start at group gq0
static int sp_block_ids_begin(debwt_ctx *c, u64 gq0, u64 groups) {
    c->route_direct = true; c->gq0 = gq0;
    ENSURE(c, c->qlist, (std::min<u64>(groups * 32, c->Btotal) + 64) * 4);
    ENSURE(c, c->qwave, ((groups + 63) / 64 + 2) * 8);
    HIPCHK(c, hipMemsetAsync(c->qwave.p, 0, 8, c->stream));
    return DEBWT_OK;
}

static int sp_flags(debwt_ctx *c, u64 g0, u64 g1) {
    int rc;
    if (g1 - g0 > (1ull << 27) - 2) { c->err = "text slice of the SP stage exceeds 2^32 positions"; return DEBWT_ERANGE; }
    c->g0 = g0; c->g1 = g1;
    const u64 ng = g1 - g0;
    if (ng && c->mzfilter && c->mztable)
        k_sp_flags<2><<<grid_for(ng, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>(
            c->text.as<u64>(), c->sepbits.as<u64>(), c->n, c->K, c->htab.as<HSlot>(), c->hbits, c->rbits.as<u32>(), c->pbits,
            c->branch.as<u64>(), c->nbranch, c->momask.as<u32>(), c->mimask.as<u32>(), g0, g1,
            sp_block_ids(c), c->branch_bitmap ? c->brbits.as<u64>() : nullptr);
    else if (ng && c->mzfilter)
        k_sp_flags<1><<<grid_for(ng, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>(
            c->text.as<u64>(), c->sepbits.as<u64>(), c->n, c->K, c->htab.as<HSlot>(), c->hbits, c->rbits.as<u32>(), c->pbits,
            c->branch.as<u64>(), c->nbranch, c->momask.as<u32>(), c->mimask.as<u32>(), g0, g1,
            sp_block_ids(c), c->branch_bitmap ? c->brbits.as<u64>() : nullptr, c->mzw);
    else if (ng)
        k_sp_flags<0><<<grid_for(ng, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>(
            c->text.as<u64>(), c->sepbits.as<u64>(), c->n, c->K, c->htab.as<HSlot>(), c->hbits, c->rbits.as<u32>(), c->pbits,
            c->branch.as<u64>(), c->nbranch, c->momask.as<u32>(), c->mimask.as<u32>(), g0, g1,
            sp_block_ids(c), c->branch_bitmap ? c->brbits.as<u64>() : nullptr);
    SpCountF fc{c->momask.as<u32>() + g0, c->mimask.as<u32>() + g0};
    if ((rc = cp_count2(c, fc, ng, cp_area(c, 0), 8, cp_area(c, 1), 10))) return rc;
    if ((rc = sync_check(c))) return rc;
    c->S_local = c->h_scalars[8];
    c->B_slice = c->h_scalars[10];
    return DEBWT_OK;
}

// routed: nullptr -> work list of the multi-in positions (mi_list); else the slice's B_slice routed blue entries go there
static int sp_emit(debwt_ctx *c, u64 sp_off, u64 *routed = nullptr, int qshift = 0) {
    const u64 ng = c->g1 - c->g0;
    c->sp_off = sp_off;
    // the SP symbol buffer grows with the slices (S is ~0.1 n, the worst case n)
    ENSURE_KEEP(c, c->spsym, sp_off + c->S_local + 64, c->shard_world > 1 ? 0 : sp_off);
    if (!routed) ENSURE(c, c->mi_list, c->B_slice * 16 + 64);
    if (ng) {
        SpEmitArgs ea{c->text.as<u64>(), c->sepbits.as<u64>(), c->n, c->K, c->momask.as<u32>(), c->mimask.as<u32>(),
                      c->spsym.as<u8>(), routed ? nullptr : c->mi_list.as<ulonglong2>(), c->g0, sp_off,
                      routed, qshift, sp_block_ids(c)};
        u32 nchunks; u64 chunk;
        plan_chunks(ng, &nchunks, &chunk);
        k_sp_emit<<<nchunks, DEBWT_BLOCK, 0, c->stream>>>(ea, ng, chunk, cp_area(c, 0), cp_area(c, 1));
    }
    return DEBWT_OK;
}

static int sp_finish(debwt_ctx *c, u64 S) {
    c->S = S;
    u64 ntriples = (S >> 6) + 3;                 // 64 symbols = 3 words; two spare groups of zeros behind the end
    ENSURE(c, c->spn, ntriples * 24);
    k_pack_sp<<<grid_for(ntriples, 256), 256, 0, c->stream>>>(c->spsym.as<u8>(), S, ntriples, c->spn.as<u64>());
    c->st.sp_len = S;
    c->stage = ST_SP;
    return DEBWT_OK;
}

extern "C" int debwt_sp_generate(debwt_ctx *c) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_CLASSIFIED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc;
    // the whole text on this context (also every shard of a "replicated scan" sharded build), slice by slice
    if ((rc = sp_prepare(c))) return rc;
    const u64 ngroups = (c->n + 31) >> 5;
    const u64 slice_groups = (c->cfg.reserved & 4194304) ? 4096ull : SP_SLICE_GROUPS;   // bit 22: slices of 2^17 positions (tests)
    u64 S = 0, Bseen = 0;
    // Blue fill without atomics when a routed entry (block id | SP index | pred) fits 64 bits: the entries of all
    // slices are collected in `blue`, sorted by block id, stripped.  Otherwise (or cfg.reserved bit 5: tests) one
    // cursor atomic per entry.
    int qbits = 1;
    while ((1ull << qbits) < c->Q) qbits++;
    const int qshift = 64 - qbits;
    const bool route_sort = c->shard_world == 1 && c->Q > 0 && c->n < (1ull << (qshift - 3)) &&
                            c->B < 0xFFFFFFF0ull - (1ull << 20) &&      // the radix passes index with 32 bits
                            !(c->cfg.reserved & 32) &&
                            !((c->cfg.reserved & 262144) && c->ranges.size() > 1);   // bit 18: by key range, as for >= 2^32 entries (tests)
    // 2^32 blue entries and more (ten genomes with an Alu-like family: 5.6 G) are beyond the 32-bit positions of the radix
    // passes as ONE array, but the blocks -- and so the blue slots -- of a key range are contiguous and fewer than 2^32: the
    // routed entries of a slice are bucketed by key range (the pass that routes entries to their shard on several GPUs) and
    // appended to their range's slots; every range is then sorted by block id on its own, over the bits in which its block
    // ids differ.  (The cursor-atomic fill this replaces took 2.3 s of a 5.0 s build, profiles/r04_bench_real10x3G_first.json.)
    const size_t P = c->ranges.size();
    bool route_ranges = !route_sort && c->shard_world == 1 && P > 1 && P <= RS_RADIX && c->Q > 0 && c->n < (1ull << (qshift - 3)) &&
                        !(c->cfg.reserved & 32);
    for (size_t i = 0; route_ranges && i < P; i++) route_ranges = c->ranges[i].B < 0xFFFFFFF0ull - (1ull << 20);
    std::vector<u64> rfill(P, 0), roffs(P + 1, 0);
    if (route_ranges) {
        std::vector<u32> qb(P + 1);
        for (size_t i = 0; i < P; i++) qb[i] = (u32)c->ranges[i].qbase;
        qb[P] = (u32)c->Q;
        ENSURE(c, c->qbounds, (P + 1) * 4);
        HIPCHK(c, hipMemcpyAsync(c->qbounds.p, qb.data(), (P + 1) * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));              // qb is host memory
    }
    c->route_direct = false;
    for (u64 g0 = 0; g0 < ngroups; g0 += slice_groups) {
        const u64 g1 = std::min(ngroups, g0 + slice_groups);
        // route_sort: pass 1 keeps the block ids of the slice's multi-in positions, pass 2 writes the routed entries
        if ((route_sort || route_ranges) && (rc = sp_block_ids_begin(c, g0, g1 - g0))) return rc;
        if ((rc = sp_flags(c, g0, g1))) return rc;
        if (route_sort) {
            if (Bseen + c->B_slice > c->B) { c->err = "multi-in positions exceed the block total"; return DEBWT_EINTERNAL; }
            if ((rc = sp_emit(c, S, c->blue.as<u64>() + Bseen, qshift))) return rc;
        } else if (route_ranges) {
            // the slice's entries as emitted, and bucketed: in the key buffers (free since the ranges were classified) when
            // those are large enough
            u64 *ta = c->keysA.as<u64>(), *tb = c->keysB.as<u64>();
            size_t tb_cap = c->keysB.cap / 8;
            if (c->keysA.cap < c->B_slice * 8 + 64) { ENSURE(c, c->blue_tmp, c->B_slice * 8 + 64); ta = c->blue_tmp.as<u64>(); }
            if (c->keysB.cap < c->B_slice * 8 + 64) { ENSURE(c, c->mi_list, c->B_slice * 8 + 64); tb = c->mi_list.as<u64>(); tb_cap = c->mi_list.cap / 8; }
            if ((rc = sp_emit(c, S, ta, qshift))) return rc;
            if (c->B_slice) {
                ENSURE(c, c->rs_over, radix_over_bytes(c->B_slice));
                RsDigit dg{};
                dg.mode = 2; dg.bounds = c->qbounds.as<u32>(); dg.nb = (u32)P; dg.tshift = qshift;
                hipError_t e = radix_partition_by_shard(c->stream, ta, nullptr, c->B_slice, tb, dg, (u32)P, radix_ws(c), roffs.data(),
                                                        false, tb_cap);
                if (e != hipSuccess) { c->err = std::string("blue entries by key range: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
                for (size_t i = 0; i < P; i++) {
                    const u64 cnt = roffs[i + 1] - roffs[i];
                    if (!cnt) continue;
                    if (rfill[i] + cnt > c->ranges[i].B) { c->err = "multi-in positions exceed a key range's block total"; return DEBWT_EINTERNAL; }
                    HIPCHK(c, hipMemcpyAsync(c->blue.as<u64>() + c->ranges[i].Bbase + rfill[i], tb + roffs[i], cnt * 8,
                                             hipMemcpyDeviceToDevice, c->stream));
                    rfill[i] += cnt;
                }
            }
        } else if ((rc = sp_emit(c, S))) return rc;
        if (c->B_slice && !route_sort && !route_ranges) {
            if (c->abs32)
                k_blue_fill<1><<<grid_for(c->B_slice, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>(
                    c->mi_list.as<ulonglong2>(), c->B_slice, c->htab.as<HSlot>(), c->hbits, c->blk_start.as<u64>(),
                    (u32)c->qbase, c->blue.as<u64>(), c->mztable ? c->K : 0);
            else
                k_blue_fill<0><<<grid_for(c->B_slice, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>(
                    c->mi_list.as<ulonglong2>(), c->B_slice, c->htab.as<HSlot>(), c->hbits, c->blk_start.as<u64>(),
                    (u32)c->qbase, c->blue.as<u64>(), c->mztable ? c->K : 0);
        }
        S += c->S_local; Bseen += c->B_slice;
    }
    if (Bseen != c->Btotal) { c->err = "multi-in positions differ from the block total"; return DEBWT_EINTERNAL; }
    if (route_ranges) {
        for (size_t i = 0; i < P; i++) {
            const debwt_ctx::KeyRange &r = c->ranges[i];
            if (rfill[i] != r.B) { c->err = "multi-in positions differ from a key range's block total"; return DEBWT_EINTERNAL; }
            if (!r.B) continue;
            u64 *reg = c->blue.as<u64>() + r.Bbase, *res = reg;
            const int span = r.Q > 1 ? bits_for(r.qbase ^ (r.qbase + r.Q - 1)) : 0;     // bits in which the range's block ids differ
            bool stripped = false;                                                     // (the last pass strips when it writes to `reg`)
            if (span) {
                ENSURE(c, c->rs_over, radix_over_bytes(r.B));
                ENSURE(c, c->rs_pair, radix_pair_bytes(r.B, qshift, std::min(64, qshift + span), true, nullptr));
                u64 *tmp = c->keysA.as<u64>();
                if (c->keysA.cap < r.B * 8 + 64) { ENSURE(c, c->blue_tmp, r.B * 8 + 64); tmp = c->blue_tmp.as<u64>(); }
                hipError_t e = hipSuccess;
                // (an odd number of passes rotates through the other key buffer, so that the last one lands -- stripped -- in `reg`)
                u64 *third = c->keysB.cap >= r.B * 8 + 64 && c->keysB.as<u64>() != tmp ? c->keysB.as<u64>() : nullptr;
                res = radix_sort_bits(c->stream, reg, tmp, r.B, qshift, std::min(64, qshift + span), radix_ws(c), &e, qshift, &stripped, third);
                if (e != hipSuccess) { c->err = std::string("blue entry sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
            }
            if (!stripped) k_blue_strip<<<grid_for(r.B, 256), 256, 0, c->stream>>>(res, reg, r.B, qshift);
        }
    }
    if (route_sort && c->B) {
        // scratch of B words: a key buffer when it is large enough (free since the ranges were classified)
        u64 *tmp;
        if (c->keysA.cap >= c->B * 8) tmp = c->keysA.as<u64>();
        else { ENSURE(c, c->blue_tmp, c->B * 8 + 64); tmp = c->blue_tmp.as<u64>(); }
        ENSURE(c, c->rs_over, radix_over_bytes(c->B));
        ENSURE(c, c->rs_pair, radix_pair_bytes(c->B, qshift, 64, true, nullptr));
        hipError_t e = hipSuccess;
        bool stripped = false;                                   // (the last pass strips when it writes to `blue`)
        u64 *third = c->keysB.cap >= c->B * 8 + 64 && c->keysB.as<u64>() != tmp ? c->keysB.as<u64>() : nullptr;
        u64 *r = radix_sort_bits(c->stream, c->blue.as<u64>(), tmp, c->B, qshift, 64, radix_ws(c), &e, qshift, &stripped, third);
        if (e != hipSuccess) { c->err = std::string("blue entry sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
        if (!stripped) k_blue_strip<<<grid_for(c->B, 256), 256, 0, c->stream>>>(r, c->blue.as<u64>(), c->B, qshift);
    }
    return sp_finish(c, S);
}

// ---------------------------------------------------------------------------------------------------
// stage 4: blue-block sort                                                                     (a-5)

// blocks above BLUE_LDS_CAP rows (see LargeSplit)
static int bitonic_large(debwt_ctx *c, u64 b0, u32 m, u64 j0) {
    u64 P = 2;
    while (P < m) P <<= 1;
    ENSURE(c, c->large_k0, P * 8);
    ENSURE(c, c->large_en, P * 8);
    k_large_load<<<grid_for(P, 256), 256, 0, c->stream>>>(c->blue.as<u64>(), b0, m, P, c->spn.as<u64>(),
                                                          c->large_k0.as<u64>(), c->large_en.as<u64>());
    for (u64 kk = 2; kk <= P; kk <<= 1)
        for (u64 jj = kk >> 1; jj > 0; jj >>= 1)
            k_large_step<<<grid_for(P >> 1, 256), 256, 0, c->stream>>>(
                c->large_k0.as<u64>(), c->large_en.as<u64>(), P, kk, jj, c->spn.as<u64>(), c->S);
    k_large_store<<<grid_for(m, 256), 256, 0, c->stream>>>(c->blue.as<u64>(), b0, m, j0, c->large_en.as<u64>(), c->mchar.as<u8>());
    return DEBWT_OK;
}

// the blocks large_q[l0, l0 + nl)
static int sort_large_blocks(debwt_ctx *c, const BlueSub &sub, u64 l0, u64 nl) {
    int rc;
    // descriptors of the large blocks: one gather, one copy
    std::vector<u64> desc3(3 * nl);
    ENSURE(c, c->large_k0, 3 * nl * 8);
    k_large_gather<<<grid_for(nl, 256), 256, 0, c->stream>>>(c->large_q.as<u32>() + l0, nl, c->blk_freq.as<u32>(),
                                                            c->blk_start.as<u64>(), c->blk_j0.as<u64>(), c->large_k0.as<u64>());
    HIPCHK(c, hipMemcpyAsync(desc3.data(), c->large_k0.p, desc3.size() * 8, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sync_check(c))) return rc;
    // rounds: every pending block is split in the same five launches (batches of at most LS_BATCH_ROWS rows of
    // scratch), one synchronisation per batch; the ranges a batch reports as still too large are the next round's
    // blocks: a range of ties one pair of windows deeper, any other range on finer splitters.  A run of one symbol or a
    // tandem repeat ties for as long as it lasts and would shed 42 SP symbols per round: a range of ties that is most of
    // its block gets a PIVOT round next (LsBlock::pivot, stage_kernels.h), which measures how far every row follows one
    // row of the block and so halves what is left of a periodic stretch -- 805 rounds became ~40 on
    // scripts/gpu_lowcomplexity.py.  The bitonic network with its symbol-by-symbol comparator is only the last resort.
    constexpr u64 LS_BATCH_ROWS = 1ull << 29;
    struct Work { u64 b0, j0; u32 m, depth, pivot; };
    std::vector<Work> work, next;
    u32 maxm = 0;
    for (u64 t = 0; t < nl; t++) {
        work.push_back(Work{desc3[3 * t], desc3[3 * t + 1], (u32)desc3[3 * t + 2], 0u, 0u});
        maxm = std::max(maxm, (u32)desc3[3 * t + 2]);
    }
    c->st.blue_max_block = std::max<u64>(c->st.blue_max_block, maxm);
    if (c->cfg.reserved & 1024) {                                  // bit 10: bitonic network only (tests)
        for (const Work &wk : work) if ((rc = bitonic_large(c, wk.b0, wk.m, wk.j0))) return rc;
        return DEBWT_OK;
    }
    std::vector<u32> res;
    std::vector<LsOver> over;
    std::vector<LsBlock> desc;
    std::vector<u32> bigidx;
    u32 round = 0;
    // sweep knobs (scripts/ls_sweep.sh), clamped: a range aims at >= 64 rows, >= 1 sample per range, and never fewer samples
    // than ranges (k_ls_splitters takes sample (b + 1) * (ns / nb) - 1: ns / nb == 0 would index below the array)
    static const u32 bin_rows = getenv("DEBWT_LS_BIN_ROWS") ? (u32)std::min(std::max(atoi(getenv("DEBWT_LS_BIN_ROWS")), 64), 1 << 20) : LS_BIN_ROWS;
    static const u32 oversample = getenv("DEBWT_LS_OVERSAMPLE") ? (u32)std::min(std::max(atoi(getenv("DEBWT_LS_OVERSAMPLE")), 1), 64) : LS_OVERSAMPLE;
    const bool trace = getenv("DEBWT_TRACE_LARGE") != nullptr;
    while (!work.empty()) {
        next.clear();
        u64 tr_rows = 0, tr_tie_n = 0, tr_tie_rows = 0, tr_piv = 0, tr_net = 0;
        for (const Work &wk : work) { tr_rows += wk.m; tr_piv += wk.pivot; }
        for (size_t w0 = 0; w0 < work.size();) {
            desc.clear(); bigidx.clear();
            u64 rows = 0, wgs = 0, slots = 0;
            u32 nbig = 0;                                          // blocks of more than 256 samples in the batch
            bool small_ns = false, big_ns = false, small_nb = false, big_nb = false;
            size_t w1 = w0;
            for (; w1 < work.size() && (desc.empty() || rows + work[w1].m <= LS_BATCH_ROWS) && wgs < 0x7FFF0000ull; w1++) {
                const Work &wk = work[w1];
                u32 nb = 8;
                while (nb < LS_MAXBINS && (u64)nb * bin_rows < wk.m) nb <<= 1;
                u32 ns = 64;
                while (ns < LS_SAMPLES && ns < nb * oversample) ns <<= 1;        // a power of two (bitonic sort), a multiple of nb
                while (nb > ns) nb >>= 1;                                          // (ns is capped at LS_SAMPLES: at least one sample per range)
                desc.push_back(LsBlock{wk.b0, wk.j0, rows, wk.m, nb, ns, (u32)wgs, (u32)slots, wk.depth, wk.pivot, ns > 256u ? nbig : 0u});
                if (ns > 256u) { bigidx.push_back((u32)(w1 - w0)); nbig++; }
                rows += (wk.m + 1u) & ~1u;
                wgs += (wk.m + LS_WG_ROWS - 1u) / LS_WG_ROWS;
                slots += nb;
                (ns <= 256u ? small_ns : big_ns) = true;
                (nb <= 64u ? small_nb : big_nb) = true;
            }
            const size_t nblk = desc.size();
            const size_t over_cap = (size_t)(rows / LS_QUEUE_CAP) + 2;
            // scratch: en (u64 per row), bin (u32 per row); per splitter slot: two splitter words, three words for each of
            // its two ranges; per block: result, descriptor; per workgroup: its block; the batch's oversize ranges
            ENSURE(c, c->ls_buf, rows * 12 + slots * 40 + (size_t)nbig * (LS_SAMPLES * 16 + 4) + nblk * (8 + sizeof(LsBlock)) + wgs * 4 +
                                     over_cap * sizeof(LsOver) + 512);
            u64 *p64 = c->ls_buf.as<u64>();
            LargeSplit ls{};
            ls.nblk = (u32)nblk;
            ls.en = p64;
            ls.spl_w = p64 + rows; ls.spl_x = ls.spl_w + slots;
            ls.smp_w = ls.spl_x + slots; ls.smp_x = ls.smp_w + (size_t)nbig * LS_SAMPLES;
            LsBlock *dblk = reinterpret_cast<LsBlock *>(ls.smp_x + (size_t)nbig * LS_SAMPLES);
            ls.blk = dblk;
            ls.over = reinterpret_cast<LsOver *>(dblk + nblk);
            ls.bin = reinterpret_cast<u32 *>(ls.over + over_cap);
            ls.cnt = ls.bin + rows; ls.start = ls.cnt + 2 * slots; ls.cur = ls.start + 2 * slots;
            ls.wgblk = ls.cur + 2 * slots;
            ls.piv = ls.wgblk + wgs;
            u32 *d_big = ls.piv + nblk;
            ls.bigidx = d_big;
            ls.res = d_big + nbig;
            ls.nover = ls.res + nblk;                               // (read back together with res)
            if (nbig) HIPCHK(c, hipMemcpyAsync(d_big, bigidx.data(), (size_t)nbig * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(dblk, desc.data(), nblk * sizeof(LsBlock), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(ls.nover, 0, 4, c->stream));
            if (small_ns) k_ls_splitters<256, 256><<<(u32)nblk, 256, 0, c->stream>>>(c->blue.as<u64>(), c->spn.as<u64>(), c->S, ls);
            if (big_ns) {
                k_ls_splitters<LS_SAMPLES, 64, 1><<<nbig, 64, 0, c->stream>>>(c->blue.as<u64>(), c->spn.as<u64>(), c->S, ls);
                k_ls_sample_keys<<<dim3(nbig, LS_SAMPLES / 256), 256, 0, c->stream>>>(c->blue.as<u64>(), c->spn.as<u64>(), c->S, ls);
                k_ls_splitters<LS_SAMPLES, 1024, 2><<<nbig, 1024, 0, c->stream>>>(c->blue.as<u64>(), c->spn.as<u64>(), c->S, ls);
            }
            k_ls_bin<<<(u32)wgs, 256, 0, c->stream>>>(c->blue.as<u64>(), c->spn.as<u64>(), c->S, ls);
            if (small_nb) k_ls_plan<64><<<(u32)nblk, 64, 0, c->stream>>>(ls, sub);
            if (big_nb) k_ls_plan<LS_MAXBINS><<<(u32)nblk, LS_MAXBINS, 0, c->stream>>>(ls, sub);
            k_ls_scatter<<<(u32)wgs, 256, 0, c->stream>>>(c->blue.as<u64>(), ls);
            res.resize(nblk + 1);
            HIPCHK(c, hipMemcpyAsync(res.data(), ls.res, (nblk + 1) * 4, hipMemcpyDeviceToHost, c->stream));
            if ((rc = sync_check(c))) return rc;                   // desc and res are host memory
            const u32 nover = res[nblk];
            if (nover > over_cap) { c->err = "large-block split: more oversize ranges than rows allow"; return DEBWT_EINTERNAL; }
            over.resize(nover);
            if (nover) HIPCHK(c, hipMemcpy(over.data(), ls.over, nover * sizeof(LsOver), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < nblk; i++)                       // sub-block table full: nothing of the block moved
                if (res[i]) { const Work &wk = work[w0 + i]; if ((rc = bitonic_large(c, wk.b0, wk.m, wk.j0))) return rc; }
            for (const LsOver &o : over) {
                const Work &wk = work[w0 + o.blk];
                if (o.ties) { tr_tie_n++; tr_tie_rows += o.cnt; }
                // a range of ties shares o.adv more pairs of windows (1 after a window round); one that is most of
                // its block is a stretch that keeps tying: pivot round next.  After a pivot round a range of ties is
                // smaller than its block (the pivot row itself is not in it), so the rounds end.
                const u64 deeper = ((u64)wk.depth + o.adv + 1) * (2 * SP_WIN);
                // (rows that left the pivot at once -- adv 0 after a pivot round -- show no such stretch: window round)
                const u32 pivot = (o.ties && (u64)o.cnt * 4 > wk.m && (!wk.pivot || o.adv >= 1) && !(c->cfg.reserved & 8192)) ? 1u : 0u;
                if (o.ties && (o.adv || wk.pivot) && deeper < c->S + 2 * SP_WIN && o.cnt < wk.m + (wk.pivot ? 0u : 1u))
                    next.push_back(Work{wk.b0 + o.st, wk.j0 + o.st, o.cnt, wk.depth + o.adv, pivot});
                else if (!o.ties && o.cnt < wk.m) next.push_back(Work{wk.b0 + o.st, wk.j0 + o.st, o.cnt, wk.depth + o.adv, wk.pivot});
                else { tr_net++; if ((rc = bitonic_large(c, wk.b0 + o.st, o.cnt, wk.j0 + o.st))) return rc; }
            }
            w0 = w1;
        }
        if (trace) {
            u32 dmax = 0; u64 rows = 0;
            for (const Work &wk : next) { dmax = std::max(dmax, wk.depth); rows += wk.m; }
            fprintf(stderr, "large blocks: round %u of %zu blocks (%llu rows, %llu pivot rounds) -> %zu ranges to split again (%llu rows, deepest %u; "
                            "ranges of ties: %llu with %llu rows; to the network: %llu)\n",
                    round, work.size(), (unsigned long long)tr_rows, (unsigned long long)tr_piv, next.size(), (unsigned long long)rows, dmax,
                    (unsigned long long)tr_tie_n, (unsigned long long)tr_tie_rows, (unsigned long long)tr_net);
        }
        work.swap(next);
        round++;
    }
    return DEBWT_OK;
}

#ifndef BLUE_QUEUE_LEVELS
#define BLUE_QUEUE_LEVELS 1            // (measured at 10 x 300 Mbp: 1, 2, 3, 4, 6 levels all give a blue stage of 19.6-20.0 ms)
#endif
// the sub-block table of a blue sort (BlueSub): the deep tie groups of the larger size classes wait there for the
// wave-per-block kernels
struct BlueQueue { BlueSub sub; u32 *count; u32 cap; };
static int blue_queue(debwt_ctx *c, BlueQueue *bq) {
    const u32 sub_cap = (u32)std::min<u64>(std::max<u64>(c->B / 8, 1u << 16), 1u << 26);
    ENSURE(c, c->sub_start, (size_t)sub_cap * 8);
    ENSURE(c, c->sub_j0, (size_t)sub_cap * 8);
    ENSURE(c, c->sub_freq, (size_t)sub_cap * 4);
    ENSURE(c, c->sub_depth, (size_t)sub_cap * 4 + 16);
    bq->cap = sub_cap;
    bq->count = c->sub_depth.as<u32>() + sub_cap;
    bq->sub = BlueSub{c->sub_start.as<u64>(), c->sub_freq.as<u32>(), c->sub_j0.as<u64>(), c->sub_depth.as<u32>(), bq->count,
                      (c->cfg.reserved & 128) ? 0u : sub_cap};      // bit 7: no hand-off (tests)
    return DEBWT_OK;
}

// Sorts the blocks [q0, q0 + nq) of the context's block table (block order is key order is row order) and, of the blocks
// above the LDS capacity, large_q[l0, l0 + nl).  A part leaves its rows final: debwt_build_to_host runs one part per key
// range and hands the rows over while the next part is sorted.
static int blue_sort_part(debwt_ctx *c, const BlueQueue &bq, u64 q0, u64 nq, u64 l0, u64 nl) {
    int rc;
    if (!nq) return DEBWT_OK;
    const u32 Q = (u32)nq;
    const u64 *bst = c->blk_start.as<u64>() + q0, *bj0 = c->blk_j0.as<u64>() + q0;
    const u32 *bfr = c->blk_freq.as<u32>() + q0;
    const BlueSub &sub = bq.sub;
    const u32 sub_cap = bq.cap;
    u32 *sub_count = bq.count;
    HIPCHK(c, hipMemsetAsync(c->sub_freq.p, 0, (size_t)sub_cap * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(sub_count, 0, 4, c->stream));
    BlueSub none{};
    u32 g1 = (u32)std::min<u64>(Q, 1u << 16);
    // blocks of up to 16 rows -- in a collection of genomes most blocks: a node's one occurrence per genome -- four to a wave
    // (cfg.reserved bit 24: a wave each, like the other blocks of up to 128 rows -- tests, A/B)
    const u32 tiny = (c->cfg.reserved & 16777216) ? 0u : 2 * BLUE_TINY;   // (17..32 rows: two to a wave)
    if (tiny) {
        k_blue_tiny<16><<<g1, 64, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q, c->spn.as<u64>(), c->S, c->mchar.as<u8>(),
                                                  nullptr, nullptr);
        k_blue_tiny<32><<<g1, 64, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q, c->spn.as<u64>(), c->S, c->mchar.as<u8>(),
                                                  nullptr, nullptr);
    }
    // small blocks are the bulk: a small LDS footprint keeps 32 single-wave workgroups per CU in flight
    k_blue_refine<64, 128, 0><<<g1, 64, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q, tiny,
                                                       c->spn.as<u64>(), c->S, c->mchar.as<u8>(), nullptr, nullptr, none);
    // 129..256 rows: one wave per block with the LDS of that capacity (9 KB per workgroup, 17 of them per CU);
    // 257..512 rows: 18 KB per block allow 8 workgroups per CU -- four waves each rather than one: these kernels wait
    // on SP gathers, what they need is waves in flight (measured at 30 Gbp: 129..512 rows by one wave and 18 KB each
    // 86 + 156 ms for blocks + queued ranges; now 6.5 + 67 and 22 + 78 ms)
    k_blue_refine<64, 256, 128><<<g1, 64, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q, 128u, c->spn.as<u64>(), c->S,
                                                         c->mchar.as<u8>(), nullptr, nullptr, sub);
    // blocks of 257 rows and more in a collection of many genomes: by classes around sampled splitters first
    // (k_blue_classify); what that finishes is marked in `done` and skipped by the kernels behind it, which take the blocks it
    // left (cfg.reserved bit 19: those kernels alone; bit 20: by classes whatever the number of such blocks -- tests)
    const bool split1024 = c->n1024 >= 1024;
    // (... or many blocks of 257..512 rows and few above: four genomes -- the four-wave network over those blocks alone took
    // 64 ms of a 654 ms build, by classes the blue stage is 78 ms instead of 116)
    const bool by_classes = split1024 || c->n512 >= 1024;
    const u8 *done = nullptr;
    if ((by_classes || (c->cfg.reserved & 1048576)) && sub.cap && !(c->cfg.reserved & 524288)) {
        ENSURE(c, c->blue_done, c->Q + 64);
        u8 *dn = c->blue_done.as<u8>() + q0;
        HIPCHK(c, hipMemsetAsync(dn, 0, Q, c->stream));
        const u32 gc = (u32)std::min<u64>(Q, 1u << 14);
        k_blue_classify<BLUE_WAVE_CAP, BLUE_WAVE_CAP><<<gc, 256, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q, 256u, c->spn.as<u64>(),
                                                                                 c->S, c->mchar.as<u8>(), sub, dn);
        k_blue_classify<1024, BLUE_WAVE_CAP><<<gc, 256, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q, (u32)BLUE_WAVE_CAP,
                                                                        c->spn.as<u64>(), c->S, c->mchar.as<u8>(), sub, dn);
        k_blue_classify<BLUE_LDS_CAP, BLUE_WAVE_CAP><<<(u32)std::min<u64>(Q, 1u << 12), 256, 0, c->stream>>>(
            c->blue.as<u64>(), bst, bfr, bj0, Q, 1024u, c->spn.as<u64>(), c->S, c->mchar.as<u8>(), sub, dn);
        done = dn;
    }
    k_blue_refine<256, BLUE_WAVE_CAP, 128><<<(u32)std::min<u64>(Q, 1u << 14), 256, 0, c->stream>>>(
        c->blue.as<u64>(), bst, bfr, bj0, Q, 256u, c->spn.as<u64>(), c->S, c->mchar.as<u8>(), nullptr, nullptr, sub, done);
    u32 g2 = (u32)std::min<u64>(Q, 1u << 12);
    // collections of many genomes put most rows into blocks of 513..1024 rows: those get a kernel of their own
    // with half the LDS footprint (four workgroups per CU instead of two); otherwise one kernel for 513..2048
    if (split1024)
        k_blue_refine<256, 1024, BLUE_WAVE_CAP><<<g2, 256, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q, (u32)BLUE_WAVE_CAP,
                                                                      c->spn.as<u64>(), c->S, c->mchar.as<u8>(), nullptr, nullptr, sub, done);
    k_blue_refine<256, BLUE_LDS_CAP, BLUE_WAVE_CAP><<<g2, 256, 0, c->stream>>>(c->blue.as<u64>(), bst, bfr, bj0, Q,
                                                                  split1024 ? 1024u : (u32)BLUE_WAVE_CAP, c->spn.as<u64>(), c->S,
                                                                  c->mchar.as<u8>(), nullptr, nullptr, sub, done);
    // heavy-tail blocks (satellite / poly-A nodes), before the queue is drained: split in HBM into ranges the LDS
    // kernels take (queued like the tie groups); what a split cannot separate goes through the bitonic network
    if (nl && (rc = sort_large_blocks(c, sub, l0, nl))) return rc;
    // the queued groups: blocks of their own that start `depth` windows in (<= 128 rows from the 512 class,
    // <= 512 rows from the 2048 class and from the split of the large blocks: LS_QUEUE_CAP)
    const u32 gs = std::min<u32>(sub_cap, 1u << 16);
    if (done) {
        // the queued groups of 129..512 rows by classes as well, one pair of windows deeper each time (two levels): what is
        // finished leaves the queue, what still ties is queued again for the wave kernels below
        u32 *snap = sub_count + 1;                                 // (a spare word behind the counter)
        for (int level = 0; level < BLUE_QUEUE_LEVELS; level++) {
            k_copy_u32<<<1, 1, 0, c->stream>>>(sub_count, snap);
            k_blue_classify<BLUE_WAVE_CAP, BLUE_WAVE_CAP><<<std::min<u32>(gs, 1u << 14), 256, 0, c->stream>>>(
                c->blue.as<u64>(), c->sub_start.as<u64>(), c->sub_freq.as<u32>(), c->sub_j0.as<u64>(), sub_cap, 128u, c->spn.as<u64>(),
                c->S, c->mchar.as<u8>(), sub, nullptr, c->sub_depth.as<u32>(), snap, c->sub_freq.as<u32>());
        }
    }
    if (tiny) {
        k_blue_tiny<16><<<gs, 64, 0, c->stream>>>(c->blue.as<u64>(), c->sub_start.as<u64>(), c->sub_freq.as<u32>(), c->sub_j0.as<u64>(),
                                                  sub_cap, c->spn.as<u64>(), c->S, c->mchar.as<u8>(), c->sub_depth.as<u32>(), sub_count);
        k_blue_tiny<32><<<gs, 64, 0, c->stream>>>(c->blue.as<u64>(), c->sub_start.as<u64>(), c->sub_freq.as<u32>(), c->sub_j0.as<u64>(),
                                                  sub_cap, c->spn.as<u64>(), c->S, c->mchar.as<u8>(), c->sub_depth.as<u32>(), sub_count);
    }
    k_blue_refine<64, 128, 0><<<gs, 64, 0, c->stream>>>(
        c->blue.as<u64>(), c->sub_start.as<u64>(), c->sub_freq.as<u32>(), c->sub_j0.as<u64>(), sub_cap, tiny,
        c->spn.as<u64>(), c->S, c->mchar.as<u8>(), c->sub_depth.as<u32>(), sub_count, none);
    k_blue_refine<64, 256, 0><<<gs, 64, 0, c->stream>>>(
        c->blue.as<u64>(), c->sub_start.as<u64>(), c->sub_freq.as<u32>(), c->sub_j0.as<u64>(), sub_cap, 128u,
        c->spn.as<u64>(), c->S, c->mchar.as<u8>(), c->sub_depth.as<u32>(), sub_count, none);
    // (257..512 queued rows are one deep tie group as a rule: four waves per block gather its windows four times as wide)
    k_blue_refine<256, BLUE_WAVE_CAP, 0><<<std::min<u32>(gs, 1u << 14), 256, 0, c->stream>>>(
        c->blue.as<u64>(), c->sub_start.as<u64>(), c->sub_freq.as<u32>(), c->sub_j0.as<u64>(), sub_cap, 256u,
        c->spn.as<u64>(), c->S, c->mchar.as<u8>(), c->sub_depth.as<u32>(), sub_count, none);
    return DEBWT_OK;
}

extern "C" int debwt_blue_sort(debwt_ctx *c) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_SP) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc;
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    c->st.blue_max_block = 0;
    if (c->Q) {
        BlueQueue bq{};
        if ((rc = blue_queue(c, &bq))) return rc;
        if ((rc = blue_sort_part(c, bq, 0, c->Q, 0, c->nlarge))) return rc;
    }
    c->stage = ST_BLUE;
    return DEBWT_OK;
}

// ---------------------------------------------------------------------------------------------------
// stage 5: assembly                                                                            (a-6)

// rows of this shard: its node instances with its special suffixes merged in (the whole BWT when not sharded)
static u64 shard_rows(const debwt_ctx *c) { return c->Mctx + (c->s1 - c->s0); }

// assembles the 8192-row blocks [b0, b1) of this shard's rows (all of them: b1 = ~0)
// The '#' rows: collections of up to 2^20 records have k_assemble append them to a list (c->hash_rows, counter in the
// spare word 6 behind the '$' row) that assemble_finish sorts; collections of more records (read sets: n is small against
// N there) mark them in hmask and find them by one counting pass over the mask words, as every collection did before.
static bool hash_rows_by_list(const debwt_ctx *c) { return c->nrec <= (1ull << 20) && !(c->cfg.reserved & 2097152); }   // bit 21: masks (tests)
static int run_assemble(debwt_ctx *c, u8 *rowsym, u64 b0 = 0, u64 b1 = ~0ull, bool collect = true) {
    const u64 rows = shard_rows(c);
    const u64 nb = (((rows + 31) >> 5) + DEBWT_BLOCK - 1) / DEBWT_BLOCK;
    b1 = std::min(b1, nb);
    if (b0 >= b1) return DEBWT_OK;
    const bool list = collect && hash_rows_by_list(c);
    k_assemble<<<(u32)(b1 - b0), DEBWT_BLOCK, 0, c->stream>>>(
        c->mchar.as<u8>(), c->Mctx, c->sprow.as<u64>() + c->s0, c->spchr.as<u8>() + c->s0, c->s1 - c->s0, rows,
        c->bwt.as<u64>(), c->hmask.as<u32>(), c->dollar.as<u64>(), rowsym, b0, list ? c->hash_rows.as<u64>() : nullptr,
        reinterpret_cast<unsigned long long *>(c->dollar.as<u64>() + 6));
    return DEBWT_OK;
}

// '#' rows of the assembled words, stage timings, stage = ST_ASSEMBLED
static int assemble_finish(debwt_ctx *c) {
    int rc;
    u64 nw = (shard_rows(c) + 31) >> 5;
    if (hash_rows_by_list(c)) {
        u64 *h_cnt = reinterpret_cast<u64 *>(&c->h_scalars[40]);                   // (8-byte aligned pair of the pinned words)
        HIPCHK(c, hipMemcpyAsync(h_cnt, c->dollar.as<u64>() + 6, 8, hipMemcpyDeviceToHost, c->stream));
        if ((rc = sync_check(c))) return rc;
        const u64 cnt = *h_cnt;
        if (cnt > c->nrec) { c->err = "more '#' rows than records"; return DEBWT_EINTERNAL; }
        c->h_scalars[9] = (u32)cnt;
        if (cnt > 1) {                                                              // ascending (src/insertCase3.c:86-97 walks the rows in order)
            ENSURE(c, c->large_k0, cnt * 8 + 64);
            ENSURE(c, c->rs_over, radix_over_bytes(cnt));
            hipError_t e = hipSuccess;
            u64 *r = radix_sort_bits(c->stream, c->hash_rows.as<u64>(), c->large_k0.as<u64>(), cnt, 0, bits_for(shard_rows(c)), radix_ws(c), &e);
            if (e != hipSuccess) { c->err = std::string("'#' row sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
            if (r != c->hash_rows.as<u64>()) HIPCHK(c, hipMemcpyAsync(c->hash_rows.p, r, cnt * 8, hipMemcpyDeviceToDevice, c->stream));
        }
    } else {
        HashRowsF fh{c->hmask.as<u32>(), c->hash_rows.as<u64>()};
        if ((rc = cp_count(c, fh, nw, cp_area(c, 0), 9))) return rc;
        if ((rc = cp_emit(c, fh, nw, cp_area(c, 0)))) return rc;
    }
    HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
    if ((rc = sync_check(c))) return rc;
    c->n_hash_local = c->h_scalars[9];
    if (c->shard_world == 1 && c->h_scalars[9] != c->nrec - 1) {
        c->err = "number of '#' rows differs from records-1";
        return DEBWT_EINTERNAL;
    }
    // stage timings
    float ms[7] = {0};
    for (int i = 0; i < 7; i++) (void)hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]);
    c->st.ms_extract = ms[0]; c->st.ms_sort = ms[1]; c->st.ms_classify = ms[2] + ms[3];
    c->st.ms_sp = ms[4]; c->st.ms_blue = ms[5]; c->st.ms_assemble = ms[6];
    (void)hipEventElapsedTime(&c->st.ms_total, c->ev[0], c->ev[7]);
    c->st.radix_pass_launches = (uint32_t)c->n_pass_events;
    c->st.radix_pass_ms = 0.f;
    for (int i = 0; i < c->n_pass_events; i++) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, c->ev_pass[i][0], c->ev_pass[i][1]);
        c->st.radix_pass_ms += t;
    }
    c->stage = ST_ASSEMBLED;
    return DEBWT_OK;
}

extern "C" int debwt_bwt_assemble(debwt_ctx *c) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_BLUE) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
    HIPCHK(c, hipMemsetAsync(c->dollar.p, 0xFF, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dollar.as<u64>() + 6, 0, 8, c->stream));
    run_assemble(c, nullptr);
    return assemble_finish(c);
}

// Device memory for a text of up to `n` symbols in `nrec` records, before the text is there.  What a cold build pays for is
// not hipMalloc's work but the driver handing out memory another process released: beyond a pool of cleared pages it
// clears on allocation, 30 ms per GiB on this system (profiles/r04_alloc_probe.txt: 6.2 s before the second 25-GiB block
// of a process started right after one that held 250 GiB) -- seconds for the ~250 GB of a 30 Gbp build, whose kernels take 1.8 s.
// A one-shot host calls this on a helper thread while it still reads and packs its input (the file size bounds n); the
// buffers are those debwt_load_text and the stages would allocate, sized as they would size them, the data-dependent ones
// (blue entries, SP code, sub-block tables) for `branching` of the positions being branching nodes (<= 0: 0.12; a text that
// needs more grows them when it gets there).  Not to be called while another call on the context is running.
extern "C" int debwt_reserve(debwt_ctx *c, uint64_t n, uint64_t nrec, double branching, unsigned flags) {
    if (!c || n < 34 || nrec == 0 || n <= nrec * (uint64_t)c->K || (flags & ~(DEBWT_RESERVE_ONE_SHOT | DEBWT_RESERVE_COMPACT))) return DEBWT_EINVAL;
    // before the text is there, and only then: the buffers below are re-allocated WITHOUT their contents, so a context that
    // holds a loaded text (or a result) would go on with a stale census over uninitialised memory
    if (c->stage >= ST_LOADED) { c->err = "debwt_reserve: the context already holds a text (reserve comes before the load)"; return DEBWT_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (branching <= 0) branching = 0.12;
    const auto t_begin = std::chrono::steady_clock::now();
    const u64 NS = nrec * (u64)c->K, M = n - NS;
    const size_t tw = (size_t)((n + 63) >> 5) + 2, bw = (size_t)(n >> 6) + 3, ngroups = (size_t)((n + 31) >> 5);
    ENSURE(c, c->text, tw * 8);
    ENSURE(c, c->sepbits, bw * 8);
    ENSURE(c, c->sep, nrec * 8);
    ENSURE(c, c->head_keys, nrec * 8);
    ENSURE(c, c->spkey, NS * 8);
    ENSURE(c, c->sprow, NS * 8);
    ENSURE(c, c->spchr, NS + 64);
    ENSURE(c, c->bwt, ngroups * 8 + 64);
    ENSURE(c, c->hmask, ngroups * 4 + 64);
    ENSURE(c, c->hash_rows, nrec * 8 + 64);
    ENSURE(c, c->mchar, (n - NS) + 64);
    ENSURE(c, c->momask, ngroups * 4 + 64);
    ENSURE(c, c->mimask, ngroups * 4 + 64);
    // the key ranges as plan_ranges will cut them: the cap from the memory that is free now plus what the context holds
    u64 cap = c->range_cap;
    if (!cap) {
        const u64 keep_n = c->n; c->n = n;
        int rc = default_range_cap(c, 30, 4 * n + (8ull << 30), 0, &cap);
        c->n = keep_n;
        if (rc) return rc;
        // A one-shot build that is being handed memory at the driver's clearing rate (the ~2 bytes per position above came
        // slower than 10 ms per GiB) is better off with more, smaller key ranges: 30 bytes per key of range workspace at
        // ~30 ms per GiB against ~34 ms per range and 30 Gbp for another first pass over the text -- the sum is least at
        // P = sqrt(0.9 s x M / 1e9 / ms per range) ranges, but never more than RS_MAX_RANGES: beyond that the first-pass
        // histograms of the ranges no longer come from one scan of the text (28 ranges at 30 Gbp: sort stage 2.1 s instead
        // of 1.0 s, profiles/r04_cli_30G.txt).  16 ranges at 30 Gbp: 54 GB of range workspace instead of 125.  The cap stays
        // with the context (debwt_set_range_cap).
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        const double gib = (double)(tw * 8 + bw * 8 + ngroups * 20 + (n - NS)) / (double)(1ull << 30);
        if ((flags & DEBWT_RESERVE_COMPACT) && (n - NS) <= 20000000000ull) {
            // (Beyond ~20 Gbp the buffers that grow with the text alone -- 3-4 bytes per base -- are half of the device's memory:
            // a run behind another of the same size waits whatever the ranges are, 30 Gbp: 10.3-10.9 s of wall time with 16 ranges,
            // 11.5 with 7, profiles/r06_cli_compact_plan.txt; the rule below stays in charge there.)
            // Key ranges of 2^29 instances whatever the allocations cost so far: the driver clears memory when it is RELEASED
            // and an allocation that is handed a block not yet cleared waits for the whole job (profiles/r06_malloc_cost.txt: 96 GB
            // right behind another process: 72 GB at once, then 2.7 s) -- the first buffers say nothing about the large ones.
            // 3.1 Gbp in 6 ranges: 28 GiB instead of 102, 158 ms per build instead of 146 (scripts/gpu_range_footprint.py).
            const u64 P = std::min<u64>(RS_MAX_RANGES, ((n - NS) + (1ull << 29) - 1) >> 29);
            const u64 want = (u64)((double)(n - NS) / (double)std::max<u64>(1, P) * 1.02) + 1;
            if (P > 1 && want < cap) { cap = std::max<u64>(want, 1ull << 26); c->range_cap = cap; c->plan_valid = false; }
        } else if ((flags & DEBWT_RESERVE_ONE_SHOT) && gib > 4.0 && secs > 0.010 * gib) {
            const double per_range_s = 0.034 * (double)n / 30e9 + 0.004;
            const double P = std::min<double>(RS_MAX_RANGES, std::sqrt(30.0 * (double)(n - NS) / 35e9 / per_range_s));
            const u64 want = (u64)((double)(n - NS) / std::max(1.0, P) * 1.02) + 1;   // (cuts fall on prefix bins: a little slack)
            if (want < cap) { cap = std::max<u64>(want, 1ull << 26); c->range_cap = cap; c->plan_valid = false; }
        }
    }
    cap = std::min<u64>(cap, 0xFFFFFFF0ull - 1);
    u64 maxM = M;
    if (M > cap) { const u64 P = (M + cap - 1) / cap, per = (M + P - 1) / P; maxM = std::min(cap, per + per / 16); }
    ENSURE(c, c->keysA, maxM * 8 + 64);
    ENSURE(c, c->keysB, maxM * 8 + 64);
    ENSURE(c, c->rs_skew, (maxM / 2048 + 2) * 4);
    ENSURE(c, c->rs_rle, radix_rle_ws_bytes(maxM));
    ENSURE(c, c->dk, maxM * 8 + 64);
    ENSURE(c, c->dstart, maxM * 4 + 64);
    ENSURE(c, c->pflag, maxM + 64);
    const u64 Best = (u64)((double)n * branching);
    ENSURE(c, c->blue, Best * 8 + 64);
    ENSURE(c, c->spsym, Best + 64);
    ENSURE(c, c->spn, ((Best >> 6) + 3) * 24);
    const u32 sub_cap = (u32)std::min<u64>(std::max<u64>(Best / 8, 1u << 16), 1u << 26);
    ENSURE(c, c->sub_start, (size_t)sub_cap * 8);
    ENSURE(c, c->sub_j0, (size_t)sub_cap * 8);
    ENSURE(c, c->sub_freq, (size_t)sub_cap * 4);
    ENSURE(c, c->sub_depth, (size_t)sub_cap * 4 + 16);
    ENSURE(c, c->qlist, (std::min<u64>(SP_SLICE_GROUPS * 32, Best) + 64) * 4);
    ENSURE(c, c->qwave, ((std::min<u64>(SP_SLICE_GROUPS, ngroups) + 63) / 64 + 2) * 8);
    return DEBWT_OK;
}

// (whole_build: the stages run back to back, no caller can ask for what lies between them)
struct WholeBuild {
    debwt_ctx *c;
    explicit WholeBuild(debwt_ctx *c_) : c(c_) { c->whole_build = true; }
    ~WholeBuild() { c->whole_build = false; }
};

extern "C" int debwt_build(debwt_ctx *c) {
    int rc;
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    c->stage = ST_LOADED;
    WholeBuild wb{c};
    if ((rc = debwt_kmer_sort_rle(c))) return rc;
    if ((rc = debwt_classify(c))) return rc;
    if ((rc = debwt_sp_generate(c))) return rc;
    if ((rc = debwt_blue_sort(c))) return rc;
    return debwt_bwt_assemble(c);
}

// debwt_build with the result handed to the host as it becomes final.  A text built in several key ranges has its
// multi-in blocks, like its rows, in key-range order: the blue sort runs range by range, the rows of a range are
// assembled as soon as its blocks are sorted and leave on a second stream while the blocks of the next range are sorted
// (at 30 Gbp: 7.5 GB of rows, 0.13 s of copy under 0.33 s of kernels; only the last range's copy is exposed).  A text
// built in one range: debwt_build, then debwt_fetch_bwt.
extern "C" int debwt_build_to_host(debwt_ctx *c, uint64_t *bwt, uint64_t *hash_rows, uint64_t *dollar_row) {
    int rc;
    if (!c || !bwt || !dollar_row || (c->nrec > 1 && !hash_rows)) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    if (c->shard_world > 1) { c->err = "sharded context: use the debwt_shard_* calls"; return DEBWT_ESTATE; }
    c->stage = ST_LOADED;
    WholeBuild wb{c};
    if ((rc = debwt_kmer_sort_rle(c))) return rc;
    if ((rc = debwt_classify(c))) return rc;
    if ((rc = debwt_sp_generate(c))) return rc;
    if (c->ranges.size() < 2 || (c->cfg.reserved & 65536)) {        // bit 16: no overlap (tests, A/B)
        if ((rc = debwt_blue_sort(c))) return rc;
        if ((rc = debwt_bwt_assemble(c))) return rc;
        return debwt_fetch_bwt(c, bwt, hash_rows, dollar_row);
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->ev_copy) HIPCHK(c, hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    HIPCHK(c, hipMemsetAsync(c->dollar.p, 0xFF, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dollar.as<u64>() + 6, 0, 8, c->stream));
    c->st.blue_max_block = 0;
    BlueQueue bq{};
    if (c->Q && (rc = blue_queue(c, &bq))) return rc;
    const u64 rows = shard_rows(c), nw = (rows + 31) >> 5;
    u64 bdone = 0;                                                    // 8192-row blocks assembled and on their way
    DrainOnError drain{c};                                            // copies into the caller's `bwt` are queued range by range
    for (size_t i = 0; i < c->ranges.size(); i++) {
        const debwt_ctx::KeyRange &r = c->ranges[i];
        if ((rc = blue_sort_part(c, bq, r.qbase, r.Q, r.l0, r.nl))) return rc;
        // rows below `final` belong to this range or an earlier one: their symbols will not change any more
        const bool last = i + 1 == c->ranges.size();
        const u64 final = last ? rows : r.Mbase + r.M + (r.s1 - c->s0);
        const u64 b1 = last ? (nw + DEBWT_BLOCK - 1) / DEBWT_BLOCK : final / ASM_ROWS;
        if (last) HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
        if (b1 > bdone) {
            run_assemble(c, nullptr, bdone, b1);
            const u64 w0 = bdone * DEBWT_BLOCK, w1 = std::min<u64>(b1 * DEBWT_BLOCK, nw);
            HIPCHK(c, hipEventRecord(c->ev_copy, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_copy, 0));
            HIPCHK(c, hipMemcpyAsync(bwt + w0, c->bwt.as<u64>() + w0, (w1 - w0) * 8, hipMemcpyDeviceToHost, c->copy_stream));
            bdone = b1;
        }
    }
    c->stage = ST_BLUE;
    if ((rc = assemble_finish(c))) return rc;                          // synchronises the context's stream
    if (c->nrec > 1)
        HIPCHK(c, hipMemcpyAsync(hash_rows, c->hash_rows.p, (c->nrec - 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dollar_row, c->dollar.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    if ((rc = sync_check(c))) return rc;
    drain.armed = false;
    return DEBWT_OK;
}

extern "C" int debwt_fetch_bwt(debwt_ctx *c, uint64_t *bwt, uint64_t *hash_rows, uint64_t *dollar_row) {
    if (!c || !bwt || !dollar_row || (c->nrec > 1 && !hash_rows)) return DEBWT_EINVAL;
    if (c->stage < ST_ASSEMBLED) return DEBWT_ESTATE;
    if (c->shard_world > 1) { c->err = "sharded context: use debwt_shard_fetch"; return DEBWT_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(bwt, c->bwt.p, (size_t)((c->n + 31) >> 5) * 8, hipMemcpyDeviceToHost, c->stream));
    if (c->nrec > 1)
        HIPCHK(c, hipMemcpyAsync(hash_rows, c->hash_rows.p, (c->nrec - 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dollar_row, c->dollar.p, 8, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c);
}

extern "C" int debwt_fetch_rows(debwt_ctx *c, uint64_t *hash_rows, uint64_t *dollar_row) {
    if (!c || !dollar_row || (c->nrec > 1 && !hash_rows)) return DEBWT_EINVAL;
    if (c->stage < ST_ASSEMBLED) return DEBWT_ESTATE;
    if (c->shard_world > 1) { c->err = "sharded context: use debwt_shard_fetch"; return DEBWT_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->nrec > 1)
        HIPCHK(c, hipMemcpyAsync(hash_rows, c->hash_rows.p, (c->nrec - 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dollar_row, c->dollar.p, 8, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c);
}

extern "C" int debwt_bwt_census(debwt_ctx *c, uint64_t counts[4]) {
    if (!c || !counts) return DEBWT_EINVAL;
    if (c->stage < ST_ASSEMBLED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    ENSURE(c, c->dollar, 64);
    u64 *d4 = c->dollar.as<u64>() + 1;                       // four spare words behind the '$' row
    HIPCHK(c, hipMemsetAsync(d4, 0, 32, c->stream));
    k_bwt_census<<<2048, DEBWT_BLOCK, 0, c->stream>>>(c->bwt.as<u64>(), shard_rows(c), d4);
    HIPCHK(c, hipMemcpyAsync(counts, d4, 32, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c);
}

extern "C" int debwt_bwt_device_ptr(debwt_ctx *c, const uint64_t **d_words) {
    if (!c || !d_words) return DEBWT_EINVAL;
    if (c->stage < ST_ASSEMBLED) return DEBWT_ESTATE;
    *d_words = c->bwt.as<uint64_t>();
    return DEBWT_OK;
}

// ---------------------------------------------------------------------------------------------------
// k-mer-prefix sharding of one build over several GPUs.  Every shard holds the whole 2-bit text;
// shard r sorts and classifies the keys of its prefix range, owns their contiguous BWT rows and their blocks.
// Host orchestration and the collectives live in debwt_amd/sharded.py.

static void shard_slice(const debwt_ctx *c, u64 *p0, u64 *p1) {
    // slices are cut at multiples of 32 positions so that the SP stage can work on whole text words
    u64 per = ((c->n / c->shard_world) >> 5) << 5;
    *p0 = per * c->shard_rank;
    *p1 = c->shard_rank + 1 == c->shard_world ? c->n : per * (c->shard_rank + 1);
}

extern "C" int debwt_shard_begin(debwt_ctx *c, int rank, int world) {
    if (!c || world < 1 || world > 255 || rank < 0 || rank >= world) return DEBWT_EINVAL;   // owner tables hold bytes, 0xFF = none
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    c->shard_rank = rank; c->shard_world = world; c->exchange = false; c->shard_planned = false;
    c->key_lo = c->key_hi = 0; c->M = c->Mctx = c->Mfull; c->Mbase = 0; c->qbase = 0; c->s0 = 0; c->s1 = c->NS;
    c->ranges.clear(); c->plan_valid = false;
    c->stage = ST_LOADED;
    return DEBWT_OK;
}

extern "C" int debwt_shard_histogram(debwt_ctx *c, uint64_t *hist4096) {
    if (!c || !hist4096) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    ENSURE(c, c->shard_hist, SHARD_BINS * 8);
    HIPCHK(c, hipMemsetAsync(c->shard_hist.p, 0, SHARD_BINS * 8, c->stream));
    // this shard counts the positions of its text slice: the census itself is data-parallel over the text
    u64 p0, p1;
    shard_slice(c, &p0, &p1);
    if (p0 & 31ull)
        k_prefix_hist<<<2048, DEBWT_BLOCK, 0, c->stream>>>(c->text.as<u64>(), c->sepbits.as<u64>(), p0, p1, c->K,
                                                            c->shard_hist.as<u64>());
    else
        k_prefix_hist_words<<<2048, DEBWT_BLOCK, 0, c->stream>>>(c->text.as<u64>(), c->sepbits.as<u64>(), p0, p1, c->K,
                                                                  c->shard_hist.as<u64>());
    HIPCHK(c, hipMemcpyAsync(hist4096, c->shard_hist.p, SHARD_BINS * 8, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c);
}

extern "C" int debwt_shard_set_range(debwt_ctx *c, uint32_t bin_lo, uint32_t bin_hi, uint64_t m_keys, uint64_t m_base) {
    if (!c || bin_lo > bin_hi || bin_hi > SHARD_BINS) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    if (m_keys > c->Mfull) return DEBWT_EINVAL;
    const int kb = 2 * c->cfg.k;                       // key bits; a bin is the top 12 of them
    bin_range_keys(bin_lo, bin_hi, kb, &c->key_lo, &c->key_hi);            // key_hi 0: no upper bound (last shard)
    c->M = c->Mctx = m_keys; c->Mbase = m_base;
    c->shard_planned = false; c->exchange = false; c->ranges.clear();
    c->stage = ST_LOADED;
    return DEBWT_OK;
}

extern "C" int debwt_shard_plan(debwt_ctx *c, const uint64_t *hist4096, uint32_t bin_lo, uint32_t bin_hi, uint64_t m_base,
                                int exchange, uint64_t caller_held_bytes, uint32_t *nranges) {
    if (!c || !hist4096 || !nranges || bin_lo > bin_hi || bin_hi > SHARD_BINS) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int kb = 2 * c->cfg.k;
    u64 m = 0;
    for (u32 b = bin_lo; b < bin_hi; b++) m += hist4096[b];
    if (m > c->Mfull) return DEBWT_EINVAL;
    bin_range_keys(bin_lo, bin_hi, kb, &c->key_lo, &c->key_hi);
    c->M = c->Mctx = m; c->Mbase = m_base;
    u64 cap = c->range_cap;
    if (!cap) {
        // range workspace per key: 30 bytes, plus the caller's send buffer in exchange mode (the receive buffer is
        // key buffer A); the later stages hold ~3.5 bytes per position of the shard's share (row symbols, blue
        // entries and their routed form, BWT) and ~1.25 bytes per position of the whole text (2-bit text, flag
        // masks, SP code and its gather buffers, node table, the concatenated BWT on the gathering rank)
        // exchange == 2 (keys rescanned, SP code and blue entries sliced): the caller's two blue-entry buffers come
        // after the sort, ~2 bytes per position of the share (8 bytes x 2 x ~0.1 multi-in positions per base); a sliced
        // SP stage (exchange != 0) keeps the block ids of the slice's multi-in positions (4 bytes each) between its passes
        // exchange == 2 since round 6: the two blue-entry buffers ARE the key buffers (debwt_shard_scratch) and the routed
        // entries sit in one of them, so what stays beside a range's workspace is what a one-GPU build holds: per position
        // of the share 1 byte of row symbols, ~1.25 of blue entries and block ids, 0.25 of rows (3 with room for denser
        // collections), per position of the text 0.6 of text, separator bits and flag masks, ~0.35 of SP code and its gather
        // buffers, ~0.3 of node table, 0.25 of concatenated rows (1.5)
        const u64 share = c->n / (u64)c->shard_world;
        int rc = exchange == 2 ? default_range_cap(c, 30, share * 3 + c->n / 2 * 3 + (8ull << 30), caller_held_bytes, &cap)
                               : default_range_cap(c, exchange == 1 ? 40 : 30, share / 2 * 7 + (exchange ? share / 2 : 0) + c->n / 4 * 5 + (8ull << 30),
                                                   caller_held_bytes, &cap);
        if (rc) return rc;
    }
    int rc = cut_ranges(c, reinterpret_cast<const u64 *>(hist4096), bin_lo, bin_hi, cap, m);
    if (rc) return rc;
    c->shard_planned = true; c->exchange = exchange == 1; c->plan_valid = false;
    c->stage = ST_LOADED;
    *nranges = (u32)c->ranges.size();
    return DEBWT_OK;
}

// Key exchange or key rescan (include/debwt_hip.h).  Per-GPU milliseconds of what differs between the two, calibrated
// on 30 Gbp builds in a process group of one (profiles/r02_v24_bench_30G_keys_*.json):
//   rescan    a first radix pass that reads the whole text and keeps one key range takes 32.3 ms per 30 Gbp read, the
//             histogram pass before it about as much                          -> 2.2 ms per Gbp read and key range
//   exchange  sort stage 2195 ms against 1230 ms: the slice is read once per round, its keys are written grouped by
//             owner, copied (208 ms of that: 6.9 ms per Gbp when the copy stays in HBM) and then take an ordinary first
//             pass                                                            -> 40 ms per Gbp of the shard's share
//             plus 8 n / world^2 bytes over every link
extern "C" int debwt_shard_key_mode(uint64_t n, int world, double link_gbytes_per_s, double *exchange_ms, double *rescan_ms) {
    if (world < 1) world = 1;
    const double link = link_gbytes_per_s > 0 ? link_gbytes_per_s : 48.0;
    const double gbp = (double)n * 1e-9, share = gbp / world;
    const double ranges = std::max(1.0, std::ceil(share / 4.29));          // < 2^32 - 2^20 keys per range
    const double t_rescan = ranges * gbp * 2.2;
    const double t_exchange = share * 40.0 + share / world * 6.9 + (world > 1 ? share / world * 8.0 / link * 1e3 : 0.0);
    if (exchange_ms) *exchange_ms = t_exchange;
    if (rescan_ms) *rescan_ms = t_rescan;
    return t_exchange < t_rescan ? DEBWT_KEYS_EXCHANGE : DEBWT_KEYS_RESCAN;
}

extern "C" int debwt_shard_ranges(debwt_ctx *c, uint32_t *bin_bounds, uint64_t *m_keys, uint32_t capacity) {
    if (!c || !bin_bounds || !m_keys) return DEBWT_EINVAL;
    if (!c->shard_planned || c->ranges.size() > capacity) return DEBWT_ESTATE;
    const int kb = 2 * c->cfg.k;
    for (size_t i = 0; i < c->ranges.size(); i++) {
        bin_bounds[i] = (u32)(c->ranges[i].key_lo >> (kb - 12));
        bin_bounds[i + 1] = c->ranges[i].key_hi ? (u32)(c->ranges[i].key_hi >> (kb - 12)) : SHARD_BINS;
        m_keys[i] = c->ranges[i].M;
    }
    return DEBWT_OK;
}

extern "C" int debwt_shard_sort_begin(debwt_ctx *c) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED || !c->shard_planned || !c->exchange) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->stage = ST_LOADED;
    int rc = sort_begin(c);
    if (rc) join_special(c);
    return rc;
}

extern "C" int debwt_shard_sort_range(debwt_ctx *c, uint32_t range, uint64_t *d_keys, uint64_t count) {
    if (!c || (!d_keys && count)) return DEBWT_EINVAL;
    if (c->stage != ST_LOADED || !c->exchange || range >= c->ranges.size()) return DEBWT_ESTATE;
    if (count != c->ranges[range].M) { c->err = "received keys differ from the census of the range"; return DEBWT_EINTERNAL; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc = sort_range(c, range, (u64 *)d_keys);
    if (rc) join_special(c);
    return rc;
}

extern "C" int debwt_shard_sort_end(debwt_ctx *c) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage != ST_LOADED || !c->exchange) return DEBWT_ESTATE;
    join_special(c);
    return sort_end(c);
}

extern "C" int debwt_shard_classify_local(debwt_ctx *c, uint64_t *nfacts, uint64_t *nblocks, uint64_t *blue_rows) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_SORTED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->local_done) {                                  // one text-fed range: its keys are still there
        if (c->ranges.size() != 1) return DEBWT_ESTATE;
        c->Q = c->B = c->nlarge = 0; c->nfacts_acc = 0; c->n1024 = 0; c->n512 = 0;
        int rc = classify_local(c);
        if (rc) return rc;
        if ((rc = append_range(c, c->ranges[0]))) return rc;
    }
    if (nfacts) *nfacts = c->nfacts_acc;
    if (nblocks) *nblocks = c->Q;
    if (blue_rows) *blue_rows = c->B;
    return DEBWT_OK;
}

extern "C" int debwt_shard_facts_export(debwt_ctx *c, uint64_t *d_dst, uint64_t capacity) {
    if (!c || !d_dst) return DEBWT_EINVAL;
    if (!c->facts_ready || capacity < c->nfacts_acc) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->nfacts_acc)
        HIPCHK(c, hipMemcpyAsync(d_dst, c->facts_acc.p, c->nfacts_acc * 8, hipMemcpyDeviceToDevice, c->stream));
    return sync_check(c);
}

extern "C" int debwt_shard_classify_global(debwt_ctx *c, const uint64_t *d_facts, uint64_t nfacts, uint64_t qbase,
                                           uint64_t blue_total) {
    if (!c || (!d_facts && nfacts)) return DEBWT_EINVAL;
    if (c->stage < ST_SORTED || !c->facts_ready) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return classify_global(c, (const u64 *)d_facts, nfacts, qbase, blue_total);
}

// ---- exchange mode: keys and blue entries travel by alltoallv, every shard scans only its text slice ----------

extern "C" int debwt_shard_partition_keys(debwt_ctx *c, const uint8_t *shard_of_bin, uint64_t *d_out, uint64_t capacity,
                                          uint64_t *offs) {
    // keys of this shard's text slice, grouped by destination shard (bucket exchange); bins whose
    // entry is 0xFF are not part of this exchange round and yield nothing
    if (!c || !shard_of_bin || !d_out || !offs) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    u64 p0, p1;
    shard_slice(c, &p0, &p1);
    bool sparse = false;
    for (u32 b = 0; b < SHARD_BINS; b++) {
        if (shard_of_bin[b] == 0xFF) sparse = true;
        else if (shard_of_bin[b] >= c->shard_world) return DEBWT_EINVAL;
    }
    if (capacity >= 0xFFFFFFF0ull) capacity = 0xFFFFFFF0ull - 1;     // a pass addresses its output with 32 bits
    ENSURE(c, c->dest_tab, SHARD_BINS);
    HIPCHK(c, hipMemcpyAsync(c->dest_tab.p, shard_of_bin, SHARD_BINS, hipMemcpyHostToDevice, c->stream));
    const int tshift = 2 * c->cfg.k - 12;
    TextKeySrc ts{c->text.as<u64>(), c->sepbits.as<u64>(), c->n, c->K, 0, 0, p0, nullptr,
                  sparse ? c->dest_tab.as<u8>() : nullptr, tshift};
    RsDigit dg{};
    dg.mode = 1; dg.tab = c->dest_tab.as<u8>(); dg.tshift = tshift;
    hipError_t e = radix_partition_by_shard(c->stream, nullptr, &ts, p1 - p0, (u64 *)d_out, dg, (u32)c->shard_world,
                                            radix_ws(c), (u64 *)offs, sparse, capacity);
    if (e == hipErrorInvalidValue && offs[c->shard_world] > capacity) {       // refused before the scatter wrote anything
        c->err = "partition output exceeds the caller's buffer";
        return DEBWT_EINTERNAL;
    }
    if (e != hipSuccess) { c->err = hipGetErrorString(e); return DEBWT_EDEVICE; }
    return DEBWT_OK;
}

// flags of the slice, in pieces of < 2^32 positions; totals of the slice
extern "C" int debwt_shard_sp_flags(debwt_ctx *c, uint64_t *sp_symbols, uint64_t *mi_positions) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_CLASSIFIED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    u64 p0, p1;
    shard_slice(c, &p0, &p1);
    int rc = sp_prepare(c);
    if (rc) return rc;
    c->sub.clear();
    c->S_rank = c->B_rank = 0;
    const u64 G0 = p0 >> 5, G1 = (p1 + 31) >> 5;
    if ((rc = sp_block_ids_begin(c, G0, G1 - G0 + 1))) return rc;     // block ids of the slice's multi-in positions
    for (u64 g0 = G0; g0 < G1 || c->sub.empty(); g0 += SP_SLICE_GROUPS) {
        const u64 g1 = std::min(G1, g0 + SP_SLICE_GROUPS);
        if ((rc = sp_flags(c, g0, g1))) return rc;
        c->sub.push_back(debwt_ctx::SubSlice{g0, g1, c->S_local, c->B_slice});
        c->S_rank += c->S_local; c->B_rank += c->B_slice;
    }
    if (sp_symbols) *sp_symbols = c->S_rank;
    if (mi_positions) *mi_positions = c->B_rank;
    return DEBWT_OK;
}

// bits of a routed blue entry: block id << qshift | SP index << 3 | pred
static int routed_qshift(const debwt_ctx *c) {
    int qbits = 1;
    while ((1ull << qbits) < c->Qtotal) qbits++;
    return 64 - qbits;
}

extern "C" int debwt_shard_sp_emit(debwt_ctx *c, uint64_t sp_offset, uint8_t *d_dst, uint64_t capacity) {
    // SP symbols of the slice at global offset sp_offset (a copy of them goes to the DEVICE buffer d_dst) and its
    // multi-in positions as routed blue entries (kept in the context for debwt_shard_blue_route)
    if (!c || !d_dst) return DEBWT_EINVAL;
    if (c->stage < ST_CLASSIFIED || c->sub.empty() || capacity < c->S_rank) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int qshift = routed_qshift(c);
    if (sp_offset + c->S_rank >= (1ull << (qshift - 3))) {
        c->err = "a routed blue entry cannot hold block id and SP index in 61 bits";
        return DEBWT_ERANGE;
    }
    // the routed entries of the slice: in key buffer A when the keys were read off the text (the buffer is free since the
    // ranges were classified; debwt_shard_scratch hands B to the caller as its send buffer and A -- after the route -- as
    // its receive buffer, so that a sliced SP stage holds no exchange buffer of its own beside the key buffers)
    u64 *routed;
    if (!c->exchange && c->keysA.cap >= c->B_rank * 8 + 64) routed = c->keysA.as<u64>();
    else { ENSURE(c, c->facts_tmp, c->B_rank * 8 + 64); routed = c->facts_tmp.as<u64>(); }
    c->routed = routed;
    u64 off = sp_offset, bseen = 0;
    int rc;
    for (const auto &sl : c->sub) {
        // the scan of the piece's flag counts again (the compaction areas hold one piece at a time)
        c->g0 = sl.g0; c->g1 = sl.g1;
        SpCountF fc{c->momask.as<u32>() + sl.g0, c->mimask.as<u32>() + sl.g0};
        if ((rc = cp_count2(c, fc, sl.g1 - sl.g0, cp_area(c, 0), 8, cp_area(c, 1), 10))) return rc;
        c->S_local = sl.S; c->B_slice = sl.B;
        if ((rc = sp_emit(c, off, routed + bseen, qshift))) return rc;
        off += sl.S; bseen += sl.B;
        if ((rc = sync_check(c))) return rc;
    }
    c->sp_off = sp_offset;
    if (c->S_rank)
        HIPCHK(c, hipMemcpyAsync(d_dst, c->spsym.as<u8>() + sp_offset, c->S_rank, hipMemcpyDeviceToDevice, c->stream));
    return sync_check(c);
}

extern "C" int debwt_shard_sp_import(debwt_ctx *c, const uint8_t *d_src, uint64_t sp_total) {
    // the SP symbols of the whole text (slices concatenated in rank order), DEVICE buffer
    if (!c || (!d_src && sp_total)) return DEBWT_EINVAL;
    if (c->stage < ST_CLASSIFIED || sp_total > c->n) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    ENSURE(c, c->spsym, sp_total + 64);
    if (sp_total) HIPCHK(c, hipMemcpyAsync(c->spsym.p, d_src, sp_total, hipMemcpyDeviceToDevice, c->stream));
    int rc = sp_finish(c, sp_total);
    if (rc) return rc;
    return sync_check(c);
}

extern "C" int debwt_shard_blue_route(debwt_ctx *c, const uint32_t *first_block_of_shard, uint64_t *d_out,
                                      uint64_t capacity, uint64_t *offs) {
    // the routed blue entries of this shard's text slice, grouped by the shard that owns their block
    if (!c || !first_block_of_shard || !d_out || !offs) return DEBWT_EINVAL;
    if (c->stage < ST_CLASSIFIED || capacity < c->B_rank) return DEBWT_ESTATE;
    if (c->B_rank >= 0xFFFFFFF0ull) { c->err = "a text slice holds 2^32 multi-in positions or more"; return DEBWT_ERANGE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const u32 w = (u32)c->shard_world;
    ENSURE(c, c->qbounds, (w + 1) * 4);
    HIPCHK(c, hipMemcpyAsync(c->qbounds.p, first_block_of_shard, (w + 1) * 4, hipMemcpyHostToDevice, c->stream));
    for (u32 i = 0; i <= w; i++) offs[i] = 0;
    if (!c->B_rank) return sync_check(c);
    RsDigit dg{};
    dg.mode = 2; dg.bounds = c->qbounds.as<u32>(); dg.nb = w; dg.tshift = routed_qshift(c);
    if (!c->routed || (u64 *)d_out == c->routed) { c->err = "blue route: no routed entries, or the output is their own buffer"; return DEBWT_ESTATE; }
    hipError_t e = radix_partition_by_shard(c->stream, c->routed, nullptr, c->B_rank, (u64 *)d_out, dg, w,
                                            radix_ws(c), (u64 *)offs, false, capacity);
    if (e != hipSuccess) { c->err = hipGetErrorString(e); return DEBWT_EDEVICE; }
    return DEBWT_OK;
}

extern "C" int debwt_shard_blue_place(debwt_ctx *c, uint64_t *d_entries, uint64_t count) {
    if (!c || (!d_entries && count)) return DEBWT_EINVAL;
    if (c->stage < ST_SP) return DEBWT_ESTATE;
    if (count != c->B) { c->err = "received blue entries differ from the rows of the owned blocks"; return DEBWT_EINTERNAL; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int qshift = routed_qshift(c);
    // As on one GPU (debwt_sp_generate): sorting the routed words by their block bits puts every entry into its block --
    // the owned blocks are a contiguous range of block ids and their blue slots the exclusive scan of their sizes -- and
    // k_blue_strip leaves pred | spIndex << 4.  The passes alternate between the caller's buffer (scratch from here on)
    // and `blue`.  (One cursor atomic and one scattered 8-byte store per entry, k_blue_place, took 177 ms for the 3.1 G
    // entries of 30 Gbp against 91 ms; it stays for entries that the 32-bit passes cannot index and for cfg.reserved
    // bit 5.)
    if (count >= 2 && count < 0xFFFFFFF0ull - (1ull << 20) && !(c->cfg.reserved & 32)) {
        ENSURE(c, c->rs_over, radix_over_bytes(count));
        ENSURE(c, c->rs_pair, radix_pair_bytes(count, qshift, 64, true, nullptr));
        // the passes of debwt_sp_generate's entry sort: bits spread evenly, the strip folded into the stores of the last one,
        // which writes `blue`; an even number of passes takes its first hop through a free key buffer
        {
            u64 *third = nullptr;
            for (DevBuf *kb : {&c->keysB, &c->keysA})
                if (!third && kb->cap >= count * 8 + 64 && kb->as<u64>() != (u64 *)d_entries && !(c->exchange && kb == &c->keysA)) third = kb->as<u64>();
            hipError_t e = hipSuccess;
            if (radix_sort_bits_into(c->stream, (u64 *)d_entries, c->blue.as<u64>(), third, count, qshift, 64, radix_ws(c), &e, qshift)) {
                if (e != hipSuccess) { c->err = std::string("blue entry sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
                return sync_check(c);
            }
        }
        u64 *src = reinterpret_cast<u64 *>(d_entries), *dst = c->blue.as<u64>();
        for (int shift = qshift; shift < 64; shift += 8) {
            hipError_t e = hipSuccess;
            u64 *r = radix_sort_bits(c->stream, src, dst, count, shift, std::min(shift + 8, 64), radix_ws(c), &e);
            if (e != hipSuccess || r != dst) { c->err = std::string("blue entry sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
            std::swap(src, dst);
        }
        k_blue_strip<<<grid_for(count, 256), 256, 0, c->stream>>>(src, c->blue.as<u64>(), count, qshift);
        return sync_check(c);
    }
    ENSURE(c, c->qcursor, c->Q * 4 + 64);
    if (c->Q) HIPCHK(c, hipMemsetAsync(c->qcursor.p, 0, c->Q * 4, c->stream));
    if (count)
        k_blue_place<<<grid_for(count, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>((const u64 *)d_entries, count,
                                                                                 (u32)c->qbase, (u32)c->Q, qshift,
                                                                                 c->qcursor.as<u32>(), c->blk_start.as<u64>(),
                                                                                 c->blue.as<u64>());
    return sync_check(c);
}

extern "C" int debwt_shard_scratch(debwt_ctx *c, int which, void **ptr, uint64_t *bytes) {
    if (!c || !ptr || !bytes || which < 0 || which > 1) return DEBWT_EINVAL;
    *ptr = nullptr; *bytes = 0;
    if (c->stage < ST_CLASSIFIED || c->exchange) return DEBWT_OK;        // exchange mode: key buffer A is the caller's own
    DevBuf &b = which == DEBWT_SCRATCH_SEND ? c->keysB : c->keysA;
    *ptr = b.p; *bytes = b.cap;
    return DEBWT_OK;
}

// Final concatenation: the shards' packed row ranges, each packed from its own first row, are
// shift-merged into the BWT words of the whole text (the reference joins its per-thread SP segments the same way,
// src/generateSP.c:379-405).  d_parts: DEVICE words of all parts; part i starts at word part_word_off[i] (one spare
// readable word behind each part), holds rows [row_base[i], row_base[i] + rows[i]); d_out: ceil(n/32) DEVICE words.
extern "C" int debwt_concat_rows(debwt_ctx *c, const uint64_t *d_parts, uint32_t nparts, const uint64_t *part_word_off,
                                 const uint64_t *row_base, const uint64_t *rows, uint64_t n, uint64_t *d_out) {
    if (!c || !d_parts || !nparts || !part_word_off || !row_base || !rows || !d_out) return DEBWT_EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::vector<ConcatPart> pp;
    u64 next = 0;
    for (u32 i = 0; i < nparts; i++) {
        if (!rows[i]) continue;
        if (row_base[i] != next) { c->err = "shard row ranges do not tile the BWT"; return DEBWT_EINVAL; }
        pp.push_back(ConcatPart{part_word_off[i], row_base[i], rows[i]});
        next += rows[i];
    }
    if (next != n) { c->err = "shard rows do not add up to n"; return DEBWT_EINVAL; }
    ENSURE(c, c->qbounds, pp.size() * sizeof(ConcatPart) + 64);
    HIPCHK(c, hipMemcpyAsync(c->qbounds.p, pp.data(), pp.size() * sizeof(ConcatPart), hipMemcpyHostToDevice, c->stream));
    const u64 nw = (n + 31) >> 5;
    k_concat_rows<<<grid_for(nw, 256), 256, 0, c->stream>>>((const u64 *)d_parts, c->qbounds.as<ConcatPart>(), (u32)pp.size(), n,
                                                            (u64 *)d_out);
    return sync_check(c);                                   // pp is host memory
}

extern "C" int debwt_shard_info(debwt_ctx *c, uint64_t *row_base, uint64_t *rows, uint64_t *hash_rows) {
    if (!c) return DEBWT_EINVAL;
    if (c->stage < ST_CLASSIFIED) return DEBWT_ESTATE;
    if (row_base) *row_base = c->Mbase + c->s0;
    if (rows) *rows = shard_rows(c);
    if (hash_rows) *hash_rows = c->n_hash_local;
    return DEBWT_OK;
}

extern "C" int debwt_shard_fetch(debwt_ctx *c, uint64_t *words, uint64_t *hash_rows, uint64_t *dollar_row) {
    // words: ceil(rows/32), row j of the shard at bit 2*(31-(j&31)) of word j>>5; hash_rows / dollar_row are
    // GLOBAL rows (dollar_row = ~0 when the '$' row is not in this shard)
    if (!c || !dollar_row) return DEBWT_EINVAL;             // words == NULL: only the row lists
    if (c->stage < ST_ASSEMBLED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const u64 rows = shard_rows(c), base = c->Mbase + c->s0;
    if (words) HIPCHK(c, hipMemcpyAsync(words, c->bwt.p, (size_t)((rows + 31) >> 5) * 8, hipMemcpyDeviceToHost, c->stream));
    if (c->n_hash_local && hash_rows)
        HIPCHK(c, hipMemcpyAsync(hash_rows, c->hash_rows.p, c->n_hash_local * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dollar_row, c->dollar.p, 8, hipMemcpyDeviceToHost, c->stream));
    int rc = sync_check(c);
    if (rc) return rc;
    for (u64 i = 0; i < c->n_hash_local && hash_rows; i++) hash_rows[i] += base;
    if (*dollar_row != ~0ull) *dollar_row += base;
    return DEBWT_OK;
}

extern "C" int debwt_pinned_alloc(size_t bytes, void **out) {
    if (!out || !bytes) return DEBWT_EINVAL;
    *out = nullptr;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? DEBWT_OK : DEBWT_ENOMEM;
}
extern "C" void debwt_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

extern "C" int debwt_shard_export(debwt_ctx *c, uint64_t *d_words, uint64_t capacity) {
    // the shard's packed rows to a DEVICE buffer (for the gather of the final concat); the words behind the last
    // row up to `capacity` are zeroed
    if (!c || !d_words) return DEBWT_EINVAL;
    if (c->stage < ST_ASSEMBLED) return DEBWT_ESTATE;
    const u64 nw = (shard_rows(c) + 31) >> 5;
    if (capacity < nw) return DEBWT_EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (nw) HIPCHK(c, hipMemcpyAsync(d_words, c->bwt.p, nw * 8, hipMemcpyDeviceToDevice, c->stream));
    if (capacity > nw) HIPCHK(c, hipMemsetAsync(d_words + nw, 0, (capacity - nw) * 8, c->stream));
    return sync_check(c);
}

extern "C" int debwt_census_words(debwt_ctx *c, const uint64_t *d_words, uint64_t n, uint64_t counts[4]) {
    if (!c || !d_words || !counts) return DEBWT_EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    u64 *d4 = c->dollar.as<u64>() + 1;
    HIPCHK(c, hipMemsetAsync(d4, 0, 32, c->stream));
    k_bwt_census<<<2048, DEBWT_BLOCK, 0, c->stream>>>((const u64 *)d_words, n, d4);
    HIPCHK(c, hipMemcpyAsync(counts, d4, 32, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c);
}

extern "C" int debwt_get_stats(const debwt_ctx *c, debwt_stats *out) {
    if (!c || !out) return DEBWT_EINVAL;
    *out = c->st;
    return DEBWT_OK;
}

// ---------------------------------------------------------------------------------------------------

extern "C" int debwt_fetch_array(debwt_ctx *c, debwt_array which, void *dst, uint64_t capacity, uint64_t *count) {
    if (!c || !count) return DEBWT_EINVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const void *src = nullptr;
    uint64_t cnt = 0, esz = 8;
    Stage need = ST_SORTED;
    std::vector<uint64_t> host;
    switch (which) {
        case DEBWT_ARR_SORTED_KEYS:
        case DEBWT_ARR_DISTINCT_KEYS:
            if (c->ranges.size() != 1) { c->err = "sorted keys are not kept by a multi-range build"; return DEBWT_ESTATE; }
            // the key buffers are scratch for the later stages (blue-entry sort), and in exchange mode they are the caller's
            if (which == DEBWT_ARR_SORTED_KEYS && (c->stage > ST_CLASSIFIED || c->exchange || c->shard_world > 1)) {
                c->err = "sorted keys are only kept until the SP stage reuses their buffer (and not by a shard)";
                return DEBWT_ESTATE;
            }
            if (which == DEBWT_ARR_SORTED_KEYS) { src = c->sk; cnt = c->M; } else { src = c->dk.p; cnt = c->D; }
            if (!src && cnt) { c->err = "the keys were released when the build ran out of memory"; return DEBWT_ESTATE; }
            break;
        case DEBWT_ARR_RED: src = c->red.p; cnt = c->R; need = ST_CLASSIFIED; break;
        case DEBWT_ARR_SP_SYMBOLS: src = c->spsym.p; cnt = c->S; esz = 1; need = ST_SP; break;
        case DEBWT_ARR_BLUE: src = c->blue.p; cnt = c->B; need = ST_SP; break;
        case DEBWT_ARR_BLUE_BOUND:
        case DEBWT_ARR_CASE3_BOUND: {
            need = ST_CLASSIFIED;
            if (c->stage < need) return DEBWT_ESTATE;
            std::vector<u32> fr(c->Q);
            std::vector<uint64_t> bs(c->Q), j0(c->Q);
            std::vector<uint64_t> sprow(c->NS);
            if (c->Q) {
                HIPCHK(c, hipMemcpy(fr.data(), c->blk_freq.p, c->Q * 4, hipMemcpyDeviceToHost));
                HIPCHK(c, hipMemcpy(bs.data(), c->blk_start.p, c->Q * 8, hipMemcpyDeviceToHost));
                HIPCHK(c, hipMemcpy(j0.data(), c->blk_j0.p, c->Q * 8, hipMemcpyDeviceToHost));
            }
            HIPCHK(c, hipMemcpy(sprow.data(), c->sprow.p, c->NS * 8, hipMemcpyDeviceToHost));
            if (which == DEBWT_ARR_BLUE_BOUND) {
                host.resize(c->Q);
                for (u64 q = 0; q < c->Q; q++) host[q] = bs[q] + fr[q] - 1;   // src/INandOut.c:359-361
            } else {
                // rows: instance j sits below every special suffix whose rank among the instances is <= j
                std::vector<uint64_t> mrank(c->NS);
                for (u64 s = 0; s < c->NS; s++) mrank[s] = sprow[s] - s;
                host.resize(2 * c->Q);
                for (u64 q = 0; q < c->Q; q++) {
                    uint64_t before = std::upper_bound(mrank.begin(), mrank.end(), j0[q]) - mrank.begin();
                    host[2 * q] = j0[q] + before;                                        // src/INandOut.c:349-352
                    host[2 * q + 1] = host[2 * q] + fr[q] - 1;
                }
            }
            cnt = host.size();
            *count = cnt;
            if (dst) memcpy(dst, host.data(), (size_t)std::min(cnt, capacity) * 8);
            return DEBWT_OK;
        }
        case DEBWT_ARR_ROW_SYMBOLS: {
            if (c->stage < ST_ASSEMBLED) return DEBWT_ESTATE;
            ENSURE(c, c->rowsym, c->n + 64);
            run_assemble(c, c->rowsym.as<u8>(), 0, ~0ull, false);      // (symbols only: the '#' rows of the build stay as they are)
            int rc = sync_check(c);
            if (rc) return rc;
            src = c->rowsym.p; cnt = c->n; esz = 1; need = ST_ASSEMBLED;
            break;
        }
        default: return DEBWT_EINVAL;
    }
    if (c->stage < need) return DEBWT_ESTATE;
    *count = cnt;
    uint64_t ncopy = std::min(cnt, capacity);
    if (dst && ncopy) {
        HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)ncopy * esz, hipMemcpyDeviceToHost, c->stream));
        return sync_check(c);
    }
    return DEBWT_OK;
}

extern "C" int debwt_kmer_count_sorted(debwt_ctx *c, uint64_t *kmers, uint64_t *counts, uint64_t capacity,
                                       uint64_t *distinct) {
    if (!c || !distinct) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int k = c->cfg.k;
    if (c->n <= c->nrec * (u64)k) return DEBWT_EINVAL;
    const u64 Mk = c->n - c->nrec * (u64)k;
    if (c->n >= 0xFFFFFFF0ull) return DEBWT_ERANGE;
    c->stage = ST_LOADED;   // the pipeline buffers are reused
    ENSURE(c, c->keysA, c->n * 8 + 64);
    ENSURE(c, c->keysB, c->n * 8 + 64);
    ENSURE(c, c->rs_skew, (c->n / 2048 + 2) * 4);
    ENSURE(c, c->dk, c->n * 8 + 64);
    ENSURE(c, c->dstart, c->n * 4 + 64);
    int rc;
    k_extract_keys<<<grid_for(c->n, DEBWT_BLOCK), DEBWT_BLOCK, 0, c->stream>>>(
        c->text.as<u64>(), c->sepbits.as<u64>(), c->sep.as<u64>(), c->nrec, c->n, k, 1, c->keysA.as<u64>());
    u64 *sorted = nullptr;
    if ((rc = sort_keys(c, c->keysA.as<u64>(), c->keysB.as<u64>(), Mk, 2 * k, &sorted, false))) return rc;
    KmerInfoF f{sorted, Mk, k, c->dk.as<u64>(), c->dstart.as<u32>()};
    if ((rc = cp_count(c, f, Mk, cp_area(c, 0), 0))) return rc;
    if ((rc = cp_emit(c, f, Mk, cp_area(c, 0)))) return rc;
    if ((rc = sync_check(c))) return rc;
    u64 D = c->h_scalars[0];
    *distinct = D;
    u64 ncopy = std::min<u64>(D, capacity);
    if (kmers && ncopy) HIPCHK(c, hipMemcpy(kmers, c->dk.p, ncopy * 8, hipMemcpyDeviceToHost));
    if (counts && ncopy) {
        std::vector<u32> first(D);
        HIPCHK(c, hipMemcpy(first.data(), c->dstart.p, D * 4, hipMemcpyDeviceToHost));
        for (u64 i = 0; i < ncopy; i++) counts[i] = (i + 1 < D ? first[i + 1] : (u32)Mk) - first[i];
    }
    return DEBWT_OK;
}

extern "C" int debwt_radix_sort_u64(debwt_ctx *c, uint64_t *d_keys, uint64_t *d_tmp, uint64_t count, int key_bits,
                                    float *ms_per_pass) {
    return debwt_radix_sort_u64_range(c, d_keys, d_tmp, count, key_bits, 0, 0, ms_per_pass);
}

extern "C" uint64_t debwt_radix_pair_passes(void) { return radix_pair_passes(); }
extern "C" uint64_t debwt_radix_bucket_passes(void) { return radix_bucket_passes(); }
extern "C" uint64_t debwt_radix_low_finishes(void) { return radix_low_finishes(); }

// keys outside [lo, hi] (a derived pass sizes the runs of its digits by the bounds: such a key would be stored outside its run)
__global__ void k_keys_outside(const u64 *__restrict__ keys, u64 n, u64 lo, u64 hi, u32 *__restrict__ flag) {
    bool bad = false;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) bad |= keys[i] < lo || keys[i] > hi;
    if (bad) *flag = 1u;
}

extern "C" int debwt_radix_sort_u64_range(debwt_ctx *c, uint64_t *d_keys, uint64_t *d_tmp, uint64_t count, int key_bits,
                                          uint64_t key_lo, uint64_t key_hi, float *ms_per_pass) {
    if (!c || !d_keys || !d_tmp || key_bits < 1 || key_bits > 64) return DEBWT_EINVAL;
    if (key_hi && key_hi <= key_lo) return DEBWT_EINVAL;
    if (count >= 0xFFFFFFF0ull) return DEBWT_ERANGE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    ENSURE(c, c->rs_skew, (count / 2048 + 2) * 4);
    ENSURE(c, c->rs_over, radix_over_bytes(count));
    const u64 range[2] = {key_lo, key_hi};
    const u64 *rg = key_lo || key_hi ? range : nullptr;
    if (rg) {
        const u64 top = key_bits >= 64 ? ~0ull : (1ull << key_bits) - 1ull;
        u32 outside = 0;
        HIPCHK(c, hipMemsetAsync(c->rs_over.p, 0, 4, c->stream));
        k_keys_outside<<<(u32)std::min<u64>(2048, (count + 255) / 256), 256, 0, c->stream>>>((const u64 *)d_keys, count, key_lo, key_hi ? key_hi - 1 : top,
                                                                                            c->rs_over.as<u32>());
        HIPCHK(c, hipMemcpyAsync(&outside, c->rs_over.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (outside) { c->err = "a key lies outside [key_lo, key_hi)"; return DEBWT_EINVAL; }
    }
    ENSURE(c, c->rs_pair, radix_pair_bytes_u64(count, key_bits, rg));
    RadixWorkspace ws = radix_ws(c);
    hipError_t e = hipSuccess;
    int np = 0;
    u64 *res = radix_sort_u64(c->stream, (u64 *)d_keys, (u64 *)d_tmp, count, key_bits, ws, c->cfg.sort_algo,
                              ms_per_pass ? &c->ev_pass[0][0] : nullptr, 16, &np, &e, nullptr, nullptr, rg);
    if (e != hipSuccess) { c->err = hipGetErrorString(e); return DEBWT_EDEVICE; }
    if (res != (u64 *)d_keys)
        HIPCHK(c, hipMemcpyAsync(d_keys, res, count * 8, hipMemcpyDeviceToDevice, c->stream));
    int rc = sync_check(c);
    if (rc) return rc;
    if (ms_per_pass) {
        float sum = 0.f;
        for (int i = 0; i < np; i++) { float t = 0.f; (void)hipEventElapsedTime(&t, c->ev_pass[i][0], c->ev_pass[i][1]); sum += t; }
        *ms_per_pass = np ? sum / np : 0.f;
    }
    return DEBWT_OK;
}

extern "C" int debwt_special_digest(const uint64_t *packed, uint64_t n, const uint64_t *sep, uint64_t nrec, int k,
                                    uint64_t digest[4]) {
    if (!packed || !sep || !digest || nrec == 0 || k < 12 || k > 32) return DEBWT_EINVAL;
    SpecialTables t;
    build_special_tables(packed, n, sep, nrec, k - 1, &t);
    auto mix = [](uint64_t h, uint64_t v) { h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); return h * 0xBF58476D1CE4E5B9ull; };
    uint64_t d[4] = {1, 2, 3, 4};
    for (uint64_t v : t.pos) d[0] = mix(d[0], v);
    for (size_t i = 0; i < t.key.size(); i++) d[1] = mix(mix(d[1], t.key[i]), t.chr[i]);
    for (uint64_t v : t.branch) d[2] = mix(d[2], v);
    for (uint64_t v : t.head_keys) d[3] = mix(d[3], v);
    for (uint64_t v : t.tail_facts) d[3] = mix(d[3], v);
    for (int i = 0; i < 4; i++) digest[i] = d[i];
    return DEBWT_OK;
}

// The special-region tables of the loaded text built twice -- on the device (special_kernels.h) and by the host module
// (special_host.cpp) -- and compared element by element: mismatch[0..5] = suffix order, keys, BWT symbols, special
// branches, head nodes, tail nodes (a table of different length counts as all of it).
extern "C" int debwt_special_compare(debwt_ctx *c, uint64_t mismatch[6]) {
    if (!c || !mismatch) return DEBWT_EINVAL;
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    join_special(c);
    if (c->nrec >= (1ull << 27) || c->NS >= (1ull << 32)) return DEBWT_ERANGE;
    // the device tables overwrite those of a build in progress: the context goes back to "loaded" (a build that follows starts
    // over and chooses its own path), and the counters of the last build stay what they were
    const debwt_stats keep = c->st;
    c->stage = ST_LOADED;
    int rc = special_device_build(c, false);
    c->special_dev = false;
    c->st = keep;
    if (rc) return rc;
    SpecialTables t;
    build_special_tables(c->h_text, c->n, c->h_sep.data(), c->nrec, c->K, &t);
    const u64 NS = c->NS, N = c->nrec;
    std::vector<u64> pos(NS), key(NS), br(c->nbranch), hk(N), tf(N);
    std::vector<u8> chr(NS);
    HIPCHK(c, hipMemcpy(pos.data(), c->sppos.p, NS * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(key.data(), c->spkey.p, NS * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(chr.data(), c->spchr.p, NS, hipMemcpyDeviceToHost));
    if (c->nbranch) HIPCHK(c, hipMemcpy(br.data(), c->branch.p, c->nbranch * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hk.data(), c->head_keys.p, N * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(tf.data(), c->tail_d.p, N * 8, hipMemcpyDeviceToHost));
    auto diff = [](const auto &a, const auto &b) {
        if (a.size() != b.size()) return (uint64_t)std::max(a.size(), b.size());
        uint64_t d = 0;
        for (size_t i = 0; i < a.size(); i++) d += a[i] != b[i];
        return d;
    };
    if (getenv("DEBWT_SPECIAL_DEBUG")) {
        int shown = 0;
        for (u64 s_ = 0; s_ < NS && shown < 12; s_++)
            if (pos[s_] != t.pos[s_]) {
                auto recof = [&](u64 p) { return (u64)(std::lower_bound(c->h_sep.begin(), c->h_sep.end(), p) - c->h_sep.begin()); };
                const u64 rd = recof(pos[s_]), rh = recof(t.pos[s_]);
                fprintf(stderr, "special mismatch at %llu: device pos %llu (rec %llu d %llu) host pos %llu (rec %llu d %llu) key %llx / %llx\n",
                        (unsigned long long)s_, (unsigned long long)pos[s_], (unsigned long long)rd, (unsigned long long)(c->h_sep[rd] - pos[s_]),
                        (unsigned long long)t.pos[s_], (unsigned long long)rh, (unsigned long long)(c->h_sep[rh] - t.pos[s_]),
                        (unsigned long long)key[s_], (unsigned long long)t.key[s_]);
                shown++;
            }
    }
    mismatch[0] = diff(pos, t.pos); mismatch[1] = diff(key, t.key); mismatch[2] = diff(chr, t.chr);
    mismatch[3] = diff(br, t.branch); mismatch[4] = diff(hk, t.head_keys); mismatch[5] = diff(tf, t.tail_facts);
    return DEBWT_OK;
}

// The checks every entry point that takes outside row lists makes before it reads a row (debwt_verify_device,
// fm_build_rank, debwt_verify_inverse): the '$' row and nrec - 1 strictly ascending '#' rows, all below n, the '$' row
// not among the '#' rows.  Returns the reason of a refusal, or NULL with *sr = the separator rows ('#' rows and the
// '$' row) ascending.
static const char *row_lists_refusal(u64 n, u64 nrec, const std::vector<u64> &hr, u64 dollar_row, std::vector<u64> *sr) {
    if (dollar_row >= n) return "'$' row outside the BWT";
    if (hr.size() != nrec - 1) return "'#' rows: nrec - 1 rows expected";
    for (size_t i = 0; i < hr.size(); i++)
        if (hr[i] >= n || (i && hr[i] <= hr[i - 1]) || hr[i] == dollar_row) return "'#' rows are not ascending rows of the BWT";
    if (sr) {
        *sr = hr;
        sr->insert(std::upper_bound(sr->begin(), sr->end(), dollar_row), dollar_row);
    }
    return nullptr;
}
// After the rank build: tot[0..3] rows per code, tot[4] separator rows, tot[5] listed rows whose code is not 3
// (k_vlisted_codes).  With that count zero every occ('T') is a difference of two counts of which the first is the
// larger, and C[3] + occ('T') stays at or below C[4].
static const char *row_census_refusal(const u64 tot[6], u64 n, u64 nrec) {
    if (tot[5]) return "a '#' row or the '$' row holds a code other than 3";
    if (tot[4] != nrec || tot[0] + tot[1] + tot[2] + tot[3] != n || tot[3] < nrec) return "rank structure: row census is inconsistent";
    return nullptr;
}

// Inverse BWT on the device (verify_kernels.h): rank structure over the packed rows, backward search for the segment
// boundaries, one LF walk per segment against the text in HBM.
extern "C" int debwt_verify_device(debwt_ctx *c, const uint64_t *d_words, const uint64_t *hash_rows, uint64_t dollar_row,
                                   uint64_t segments, debwt_verify_report *rep) {
    if (!c || !rep) return DEBWT_EINVAL;
    memset(rep, 0, sizeof *rep);
    if (c->stage < ST_LOADED) return DEBWT_ESTATE;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const u64 n = c->n, nrec = c->nrec;
    std::vector<u64> hr;
    if (!d_words) {                                           // the context's own result
        if (c->stage < ST_ASSEMBLED || c->shard_world > 1) return DEBWT_ESTATE;
        d_words = c->bwt.as<uint64_t>();
        hr.resize(nrec);
        if (nrec > 1) HIPCHK(c, hipMemcpy(hr.data(), c->hash_rows.p, (nrec - 1) * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&dollar_row, c->dollar.p, 8, hipMemcpyDeviceToHost));
        hr.resize(nrec - 1);
    } else {
        if (nrec > 1 && !hash_rows) return DEBWT_EINVAL;
        hr.assign(hash_rows, hash_rows + (nrec - 1));
    }
    std::vector<u64> sr;
    if (const char *why = row_lists_refusal(n, nrec, hr, dollar_row, &sr)) { c->err = why; return DEBWT_EINVAL; }
    // rank structure
    const u64 nlines = n / VB_ROWS + 1, nchunks = (nlines + VB_CHUNK - 1) / VB_CHUNK;
    const size_t idx_bytes = (size_t)nlines * VB_LINE * 8;
    u64 *idx;
    if (c->keysB.cap >= idx_bytes) idx = c->keysB.as<u64>();              // free between builds
    else if (c->keysA.cap >= idx_bytes) idx = c->keysA.as<u64>();
    else { ENSURE(c, c->vidx, idx_bytes); idx = c->vidx.as<u64>(); }
    if (!segments) segments = std::min<u64>(std::max<u64>(n / 16384, 1), 1ull << 20);
    const u64 gap = std::max<u64>(n / segments, 2);
    const u64 nbound = n > 2 ? (n - 2) / gap : 0;                          // (j + 1) * gap < n - 1
    const u32 maxm = (u32)std::min<u64>(std::max<u64>(gap / 2, 1), 1u << 16);
    // small arrays: [csum 5 x nchunks][totals 8][counters 8][hash nrec][srows nrec + 1][bounds 2 x (nbound + 2)]
    const size_t small_words = (size_t)nchunks * 5 + 16 + 2 * nrec + 2 + 2 * (nbound + 2) + 8;
    ENSURE(c, c->vtmp, small_words * 8);
    u64 *csum = c->vtmp.as<u64>(), *totals = csum + nchunks * 5, *counters = totals + 8, *d_hash = counters + 8,
        *d_srows = d_hash + nrec, *d_bounds = d_srows + nrec + 1;
    HIPCHK(c, hipMemsetAsync(totals, 0, 16 * 8, c->stream));
    if (!hr.empty()) HIPCHK(c, hipMemcpyAsync(d_hash, hr.data(), hr.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_srows, sr.data(), sr.size() * 8, hipMemcpyHostToDevice, c->stream));
    hipEvent_t ev[4];
    for (auto &e : ev) HIPCHK(c, hipEventCreate(&e));
    auto drop_events = [&]() { for (auto &e : ev) (void)hipEventDestroy(e); };
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    const u64 *bw = reinterpret_cast<const u64 *>(d_words);
    k_vidx_count<<<(u32)nchunks, VB_CHUNK, 0, c->stream>>>(bw, n, nlines, d_srows, sr.size(), csum);
    k_vidx_scan<<<1, 1024, 0, c->stream>>>(csum, nchunks, totals);
    k_vidx_write<<<(u32)nchunks, VB_CHUNK, 0, c->stream>>>(bw, n, nlines, d_srows, sr.size(), csum, idx);
    k_vlisted_codes<<<grid_for(sr.size(), 256), 256, 0, c->stream>>>(bw, d_srows, sr.size(), totals + 5);
    u64 tot[6];
    HIPCHK(c, hipMemcpyAsync(tot, totals, 48, hipMemcpyDeviceToHost, c->stream));
    int rc = sync_check(c);
    if (rc) { drop_events(); return rc; }
    if (const char *why = row_census_refusal(tot, n, nrec)) { drop_events(); c->err = why; return DEBWT_EINVAL; }
    VIndex V{};
    V.idx = idx; V.hash = d_hash; V.srows = d_srows; V.nhash = hr.size(); V.nsep = sr.size(); V.n = n;
    V.C[0] = 0; V.C[1] = tot[0]; V.C[2] = tot[0] + tot[1]; V.C[3] = V.C[2] + tot[2];
    V.C[4] = V.C[3] + (tot[3] - nrec); V.C[5] = n - 1;
    V.dollar_row = dollar_row;
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    // segment boundaries by backward search
    std::vector<u64> found(2 * nbound), bounds;
    if (nbound) {
        k_vsearch<<<grid_for(nbound, 256), 256, 0, c->stream>>>(V, c->text.as<u64>(), c->sepbits.as<u64>(), nbound, gap, maxm,
                                                               d_bounds, counters);
        HIPCHK(c, hipMemcpyAsync(found.data(), d_bounds, nbound * 16, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipEventRecord(ev[2], c->stream));
    if ((rc = sync_check(c))) { drop_events(); return rc; }
    bounds.push_back(0); bounds.push_back(dollar_row);
    u64 last = 0;
    for (u64 j = 0; j < nbound; j++)
        if (found[2 * j] != ~0ull && found[2 * j] > last && found[2 * j] < n - 1) {
            bounds.push_back(found[2 * j]); bounds.push_back(found[2 * j + 1]);
            last = found[2 * j];
        }
    bounds.push_back(n - 1); bounds.push_back(n - 1);                      // the suffix "$" is the last row
    const u64 nseg = bounds.size() / 2 - 1;
    HIPCHK(c, hipMemcpyAsync(d_bounds, bounds.data(), bounds.size() * 8, hipMemcpyHostToDevice, c->stream));
    k_vwalk<<<grid_for(nseg, 256), 256, 0, c->stream>>>(V, c->text.as<u64>(), c->sepbits.as<u64>(), d_bounds, nseg, counters);
    HIPCHK(c, hipEventRecord(ev[3], c->stream));
    u64 ctr[8];
    HIPCHK(c, hipMemcpyAsync(ctr, counters, 64, hipMemcpyDeviceToHost, c->stream));
    if ((rc = sync_check(c))) { drop_events(); return rc; }                 // bounds is host memory
    (void)hipEventElapsedTime(&rep->ms_index, ev[0], ev[1]);
    (void)hipEventElapsedTime(&rep->ms_search, ev[1], ev[2]);
    (void)hipEventElapsedTime(&rep->ms_walk, ev[2], ev[3]);
    drop_events();
    rep->segments = nseg; rep->steps = ctr[4]; rep->mismatches = ctr[0]; rep->broken_links = ctr[1];
    rep->search_failures = ctr[2]; rep->search_steps = ctr[3];
    rep->ok = (ctr[0] == 0 && ctr[1] == 0 && ctr[2] == 0 && ctr[4] == n - 1) ? 1 : 0;
    return DEBWT_OK;
}

extern "C" int debwt_verify_inverse(const uint64_t *bwt, uint64_t n, const uint64_t *hash_rows, uint64_t nrec,
                                    uint64_t dollar_row, uint8_t *sym_out) {
    // LF(i) = C[c] + occ(c, i); '#' rows map in order to rows n-nrec.., '$' row to row n-1
    // (src/LFsearch.c:49-166, src/insertCase3.c:141-194).  The reference walks the whole text as one chain of n
    // dependent steps; here every record is walked by its own thread: the walk that starts at the row of
    // the j-th '#' suffix (row n - nrec + j) spells the record in front of that '#' backwards and stops at the row that
    // carries the previous separator, which names the walk that precedes it in the text.
    if (!bwt || !sym_out || n < 2 || nrec < 1 || nrec > n || (nrec > 1 && !hash_rows)) return DEBWT_EINVAL;
    std::vector<u64> hr, sr;
    if (nrec > 1) hr.assign(hash_rows, hash_rows + (nrec - 1));
    if (row_lists_refusal(n, nrec, hr, dollar_row, &sr)) return DEBWT_EINVAL;
    std::vector<uint8_t> L(n);
    for (uint64_t j = 0; j < n; j++) L[j] = (uint8_t)((bwt[j >> 5] >> ((31 - (j & 31)) << 1)) & 3);
    for (u64 r : sr)
        if (L[r] != 3) return DEBWT_EINVAL;                    // the format stores code 3 under '#' and '$' (k_vlisted_codes)
    for (u64 r : hr) L[r] = 4;
    L[dollar_row] = 5;
    uint64_t C[7] = {0}, cnt[6] = {0}, seen[6] = {0};
    for (uint64_t i = 0; i < n; i++) cnt[L[i]]++;
    for (int s = 0; s < 6; s++) C[s + 1] = C[s] + cnt[s];
    if (cnt[4] != nrec - 1 || cnt[5] != 1) return DEBWT_EINTERNAL;
    std::vector<uint64_t> lf(n);
    for (uint64_t i = 0; i < n; i++) lf[i] = C[L[i]] + seen[L[i]]++;
    // walk w (0 .. nrec-1) starts at row C[4] + w: the '#' suffixes in row order, then the '$' suffix (row n-1)
    struct Walk { std::vector<uint8_t> rev; int64_t prev = -2; bool ok = false; };
    std::vector<Walk> walks(nrec);
    std::atomic<uint64_t> next_walk{0};
    auto worker = [&]() {
        for (;;) {
            uint64_t w = next_walk.fetch_add(1);
            if (w >= nrec) return;
            Walk &wk = walks[w];
            uint64_t row = C[4] + w;
            for (uint64_t steps = 0; steps <= n; steps++) {
                uint8_t sy = L[row];
                if (sy == 5) { wk.prev = -1; wk.ok = true; break; }                    // the text's first record
                if (sy == 4) { wk.prev = (int64_t)(lf[row] - C[4]); wk.ok = true; break; }
                wk.rev.push_back(sy);
                row = lf[row];
            }
        }
    };
    {
        unsigned nt = std::max(1u, std::min<unsigned>((unsigned)std::min<uint64_t>(nrec, 64), std::thread::hardware_concurrency()));
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back(worker);
        worker();
        for (auto &x : th) x.join();
    }
    // chain the records from the last one (the '$' walk) to the first
    uint64_t p = n;
    int64_t w = (int64_t)nrec - 1;
    for (uint64_t r = 0; r < nrec; r++) {
        if (w < 0 || (uint64_t)w >= nrec || !walks[w].ok) return DEBWT_EINTERNAL;
        const Walk &wk = walks[w];
        if (p < wk.rev.size() + 1) return DEBWT_EINTERNAL;
        sym_out[--p] = (r == 0) ? 5 : 4;                                               // the separator behind the record
        for (size_t i = 0; i < wk.rev.size(); i++) sym_out[--p] = wk.rev[i];
        w = wk.prev;
    }
    return (p == 0 && w == -1) ? DEBWT_OK : DEBWT_EINTERNAL;
}

// ---------------------------------------------------------------------------------------------------
// FM-index over built rows (fm_kernels.h): the verifier's rank structure, a row-sampled suffix array written by the
// verifier's walk, batched count and locate.  The index owns its memory and stream and outlives the context.

struct debwt_fm {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    u64 n = 0, nrec = 0, s = 32, nsamp = 0, dollar_row = 0;
    u32 sh = 5;
    u64 census[4]{};
    DevBuf idx, rowlists, sa;    // rank lines; '#' rows then separator rows; samples
    DevBuf q_chars, q_off, q_out, q_runs;   // query scratch, bounded by the batch sizes below
    DevBuf s_items[FM_SEARCH_MAX_K + 1], s_hits, s_ctr, s_plist;   // search scratch: levels 1..K, hits, counters
    debwt_fm_search_stats s_stats{};
    DevBuf m_slot, m_cnt, m_obase, m_spans, m_ranges, m_cspans, m_cranges;   // MEM scratch: slots, then compacted
    debwt_fm_mems_stats m_stats{};
    DevBuf text;                 // the 2-bit text (debwt_fm_attach_text); has_text: checked against the samples
    bool has_text = false;
    DevBuf x_jobs, x_best, x_cells, x_flags, x_tr, x_cigoff, x_cig;   // extension scratch of one batch
    DevBuf x_anchors;            // the anchors of one batch of chain jobs
    debwt_fm_extend_stats x_stats{};
    debwt_fm_map_stats map_stats{};
    debwt_fm_pair_stats pair_stats{};
    DevBuf o_table;              // overlaps: record and length per entry of srows, made by the first debwt_fm_overlaps
    bool has_otable = false;
    DevBuf o_slot, o_runs, o_nruns, o_nhits, o_rbase, o_hbase, o_cruns, o_rout, o_hits;   // overlap scratch of one batch
    debwt_fm_overlaps_stats o_stats{};
    debwt_fm_overlaps_mm_stats om_stats{};   // overlaps with mismatches: scratch is s_items, s_hits (runs), o_cruns, o_rout, o_hits
    DevBuf anchors;              // extract: sample numbers ordered by position, made by the first extract or restore
    bool has_anchors = false;
    u64 na = 0;                  // anchors: the samples and the free ends (0, '$' row), (n - 1, n - 1) where not sampled
    float ms_anchors = 0.f;
    DevBuf e_jobs, e_seg, e_out, e_ctr, e_sep;   // extract scratch of one batch; counters; separator positions of a restore
    debwt_fm_extract_stats e_stats{};
    DevBuf k_table;              // k-mers: [lo, hi) of every q-mer, made by the first call that needs it (k_q: its q)
    bool has_ktable = false;
    u32 k_q = 0;
    DevBuf k_coff, k_counts, k_ctr, k_active, k_info, k_ntr, k_trials, k_trun, k_res;   // k-mer and correction scratch of one batch
    debwt_fm_kmer_stats k_stats{};
    debwt_fm_correct_stats c_stats{};
    DevBuf sp_front, sp_codes, sp_mults, sp_ctr, sp_hist, sp_gsum;   // spectrum: two frontiers, list staging, counters, histogram, granule sums
    debwt_fm_spectrum_stats sp_stats{};
    DevBuf esa_lcp, esa_sa, esa_da;   // the kept arrays of debwt_fm_esa_build, allocated exactly (has_esa: counted in device_bytes)
    bool has_esa = false;
    debwt_fm_esa_summary esa_sum{};
    std::vector<u64> esa_distinct;    // the profile of the build, k = 1 .. 4096
    debwt_fm_esa_stats esa_stats{};
    debwt_fm_repeat_stats rp_stats{};
    DevBuf rec_P;                     // the kept prefix of debwt_fm_records_build, 8 n bytes exactly (counted in device_bytes)
    debwt_fm_records_stats rc_stats{};
    debwt_fm_cdbg_stats dbg_stats{};
    debwt_fm_cdbg_both_stats bidbg_stats{};
    DevBuf g_coff, g_state, g_hbase, g_raw, g_flag, g_deg, g_oseg, g_edges, g_eoff, g_len, g_keep, g_out, g_ctr;   // string graph
    debwt_fm_graph_stats g_stats{};
    DevBuf b_state, b_self, b_row, b_cnt, b_whb, b_rawbase, b_tbase, b_pos, b_aoff, b_mm, b_cur, b_cat, b_ctr;   // graph over both strands
    debwt_fm_graph_both_stats b_stats{};
    DevBuf cl_state, cl_src, cl_cnt, cl_toff, cl_tin, cl_snap, cl_mark, cl_ctr;   // graph cleaning; edges and offsets in g_edges, g_eoff
    debwt_fm_clean_stats cl_stats{};
    DevBuf p_table;              // pileup: the table of the window [p_wbeg, p_wend), 32 bytes per position
    bool has_ptable = false;
    u64 p_wbeg = 0, p_wend = 0;
    DevBuf p_codes, p_aln, p_coff, p_cig, p_span, p_ctr, p_sep, p_calls, p_vcnt, p_vbase, p_vars;   // pileup scratch of one call
    debwt_fm_pile_stats p_stats{};
    VIndex V{};
    std::vector<u64> rec_starts;
    float ms_rank = 0.f, ms_samples = 0.f;
};

namespace {

constexpr u64 FM_BATCH_PATTERNS = 1ull << 20;       // patterns per count launch
constexpr u64 FM_BATCH_CHARS = 64ull << 20;         // pattern bytes per count launch (a longer single pattern goes alone)
constexpr u64 FM_BATCH_HITS = 1ull << 22;           // occurrences per locate launch

int fm_ensure(debwt_fm *f, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return DEBWT_OK;
    HIPCHK(f, hipStreamSynchronize(f->stream));
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 4 + 256;
    HIPCHK(f, hipMalloc(&b.p, want));
    b.cap = want;
    return DEBWT_OK;
}
#define FM_ENSURE(f, b, bytes) do { int r_ = fm_ensure((f), (b), (bytes)); if (r_) return r_; } while (0)

int fm_sync(debwt_fm *f) {
    HIPCHK(f, hipStreamSynchronize(f->stream));
    HIPCHK(f, hipGetLastError());
    return DEBWT_OK;
}

// the two events a call times its launches with, destroyed on every way out
struct FmEvents {
    hipEvent_t a = nullptr, b = nullptr;
    ~FmEvents() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    int init(debwt_fm *f) { HIPCHK(f, hipEventCreate(&a)); HIPCHK(f, hipEventCreate(&b)); return DEBWT_OK; }
};

// a temporary device buffer, released on every way out
struct FmTmp {
    void *p = nullptr;
    ~FmTmp() { if (p) (void)hipFree(p); }
};

int fm_new(int device, u64 n, u64 nrec, u32 sa_sample, debwt_fm **out, std::string *err) {
    if (!sa_sample) sa_sample = 32;
    if (sa_sample > 1024 || (sa_sample & (sa_sample - 1))) { *err = "sa_sample must be a power of two in 1..1024"; return DEBWT_EINVAL; }
    if (n < 2 || nrec < 1 || nrec > n) { *err = "FM-index: n or nrec out of range"; return DEBWT_EINVAL; }
    auto *f = new (std::nothrow) debwt_fm;
    if (!f) return DEBWT_ENOMEM;
    f->device = device; f->n = n; f->nrec = nrec; f->s = sa_sample;
    f->sh = 0;
    while ((1ull << f->sh) < sa_sample) f->sh++;
    f->nsamp = (n + sa_sample - 1) / sa_sample;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { *err = std::string("FM-index stream: ") + hipGetErrorString(e); delete f; return DEBWT_EDEVICE; }
    *out = f;
    return DEBWT_OK;
}

// rank structure of packed rows in HBM (d_words, n rows) with the given '#' rows and '$' row: f->idx, f->rowlists, f->V
int fm_build_rank(debwt_fm *f, const u64 *d_words, const std::vector<u64> &hr, u64 dollar_row) {
    const u64 n = f->n, nrec = f->nrec;
    std::vector<u64> sr;
    if (const char *why = row_lists_refusal(n, nrec, hr, dollar_row, &sr)) { f->err = why; return DEBWT_EINVAL; }
    const u64 nlines = n / VB_ROWS + 1, nchunks = (nlines + VB_CHUNK - 1) / VB_CHUNK;
    FM_ENSURE(f, f->idx, (size_t)nlines * VB_LINE * 8);
    FM_ENSURE(f, f->rowlists, (size_t)(2 * nrec + 1) * 8);
    u64 *d_hash = f->rowlists.as<u64>(), *d_srows = d_hash + nrec;
    FmTmp tmp;
    HIPCHK(f, hipMalloc(&tmp.p, ((size_t)nchunks * 5 + 8) * 8));
    u64 *csum = reinterpret_cast<u64 *>(tmp.p), *totals = csum + nchunks * 5;
    if (!hr.empty()) HIPCHK(f, hipMemcpyAsync(d_hash, hr.data(), hr.size() * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(d_srows, sr.data(), sr.size() * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(totals, 0, 64, f->stream));
    hipEvent_t e0, e1;
    HIPCHK(f, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); f->err = "hipEventCreate"; return DEBWT_EDEVICE; }
    (void)hipEventRecord(e0, f->stream);
    k_vidx_count<<<(u32)nchunks, VB_CHUNK, 0, f->stream>>>(d_words, n, nlines, d_srows, sr.size(), csum);
    k_vidx_scan<<<1, 1024, 0, f->stream>>>(csum, nchunks, totals);
    k_vidx_write<<<(u32)nchunks, VB_CHUNK, 0, f->stream>>>(d_words, n, nlines, d_srows, sr.size(), csum, f->idx.as<u64>());
    (void)hipEventRecord(e1, f->stream);
    k_vlisted_codes<<<grid_for(sr.size(), 256), 256, 0, f->stream>>>(d_words, d_srows, sr.size(), totals + 5);
    u64 tot[6];
    HIPCHK(f, hipMemcpyAsync(tot, totals, 48, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (!rc) (void)hipEventElapsedTime(&f->ms_rank, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (const char *why = row_census_refusal(tot, n, nrec)) { f->err = why; return DEBWT_EINVAL; }
    for (int q = 0; q < 4; q++) f->census[q] = tot[q];
    VIndex &V = f->V;
    V = VIndex{};
    V.idx = f->idx.as<u64>(); V.hash = d_hash; V.srows = d_srows; V.nhash = hr.size(); V.nsep = sr.size(); V.n = n;
    V.C[0] = 0; V.C[1] = tot[0]; V.C[2] = tot[0] + tot[1]; V.C[3] = V.C[2] + tot[2];
    V.C[4] = V.C[3] + (tot[3] - nrec); V.C[5] = n - 1;
    V.dollar_row = dollar_row;
    f->dollar_row = dollar_row;
    return DEBWT_OK;
}

// positions of the rows of `runs` (host: first row, count) into host `out` (sum of the counts), in run order
int fm_locate_runs(debwt_fm *f, const std::vector<u64> &run_row, const std::vector<u64> &run_cnt, u64 *out) {
    const u64 nr = run_row.size();
    if (!nr) return DEBWT_OK;
    std::vector<u64> run_out(nr + 1, 0);
    for (u64 k = 0; k < nr; k++) run_out[k + 1] = run_out[k] + run_cnt[k];
    const u64 total = run_out[nr];
    if (!total) return DEBWT_OK;
    FM_ENSURE(f, f->q_runs, (size_t)(2 * nr + 1) * 8);
    u64 *d_row = f->q_runs.as<u64>(), *d_out_off = d_row + nr;
    HIPCHK(f, hipMemcpyAsync(d_row, run_row.data(), nr * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(d_out_off, run_out.data(), (nr + 1) * 8, hipMemcpyHostToDevice, f->stream));
    FM_ENSURE(f, f->q_out, (size_t)std::min(total, FM_BATCH_HITS) * 8);
    for (u64 g0 = 0; g0 < total; g0 += FM_BATCH_HITS) {
        const u64 cnt = std::min(total - g0, FM_BATCH_HITS);
        k_fm_locate<<<grid_for(cnt, 256), 256, 0, f->stream>>>(f->V, f->sa.as<u64>(), f->sh, d_row, d_out_off, nr, g0, cnt,
                                                              f->q_out.as<u64>());
        HIPCHK(f, hipMemcpyAsync(out + g0, f->q_out.p, cnt * 8, hipMemcpyDeviceToHost, f->stream));
        int rc = fm_sync(f);
        if (rc) return rc;
    }
    return DEBWT_OK;
}

// first text position of every record: the rows of the '#' suffixes (C[4] .. C[4] + nrec - 2) located, sorted, + 1
int fm_record_starts_build(debwt_fm *f) {
    std::vector<u64> pos(f->nrec - 1);
    if (f->nrec > 1) {
        int rc = fm_locate_runs(f, {f->V.C[4]}, {f->nrec - 1}, pos.data());
        if (rc) return rc;
    }
    std::sort(pos.begin(), pos.end());
    f->rec_starts.assign(1, 0);
    for (u64 p : pos) {
        if (p + 1 >= f->n) { f->err = "'#' suffix located outside the text"; return DEBWT_EINVAL; }
        f->rec_starts.push_back(p + 1);
    }
    return DEBWT_OK;
}

int fm_upload_rows(debwt_fm *f, const uint64_t *rows, FmTmp *tmp, const u64 **d_words) {
    const size_t bytes = (size_t)((f->n + 31) >> 5) * 8;
    HIPCHK(f, hipMalloc(&tmp->p, bytes));
    HIPCHK(f, hipMemcpyAsync(tmp->p, rows, bytes, hipMemcpyHostToDevice, f->stream));
    *d_words = reinterpret_cast<const u64 *>(tmp->p);
    return DEBWT_OK;
}

}  // namespace

static int fm_create_impl(debwt_ctx *c, debwt_fm *f, const uint64_t *rows, std::vector<u64> &hr, u64 dollar_row) {
    const u64 n = f->n;
    FmTmp rows_tmp;
    const u64 *d_words;
    if (!rows) d_words = c->bwt.as<u64>();
    else { int rc = fm_upload_rows(f, rows, &rows_tmp, &d_words); if (rc) return rc; }
    int rc = fm_build_rank(f, d_words, hr, dollar_row);
    if (rc) return rc;
    // segment boundaries by backward search of the loaded text (as debwt_verify_device), then the walk with the samples
    const u64 segments = std::min<u64>(std::max<u64>(n / 16384, 1), 1ull << 20);
    const u64 gap = std::max<u64>(n / segments, 2);
    const u64 nbound = n > 2 ? (n - 2) / gap : 0;
    const u32 maxm = (u32)std::min<u64>(std::max<u64>(gap / 2, 1), 1u << 16);
    FmTmp small;
    HIPCHK(f, hipMalloc(&small.p, (size_t)(8 + 2 * (nbound + 2)) * 8));
    u64 *counters = reinterpret_cast<u64 *>(small.p), *d_bounds = counters + 8;
    HIPCHK(f, hipMemsetAsync(counters, 0, 64, f->stream));
    FM_ENSURE(f, f->sa, (size_t)f->nsamp * 8);
    HIPCHK(f, hipMemsetAsync(f->sa.p, 0xFF, (size_t)f->nsamp * 8, f->stream));
    hipEvent_t e0, e1;
    HIPCHK(f, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); f->err = "hipEventCreate"; return DEBWT_EDEVICE; }
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    (void)hipEventRecord(e0, f->stream);
    std::vector<u64> found(2 * nbound), bounds;
    if (nbound) {
        k_vsearch<<<grid_for(nbound, 256), 256, 0, f->stream>>>(f->V, c->text.as<u64>(), c->sepbits.as<u64>(), nbound, gap, maxm,
                                                               d_bounds, counters);
        HIPCHK(f, hipMemcpyAsync(found.data(), d_bounds, nbound * 16, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
    }
    bounds.push_back(0); bounds.push_back(dollar_row);
    u64 last = 0;
    for (u64 j = 0; j < nbound; j++)
        if (found[2 * j] != ~0ull && found[2 * j] > last && found[2 * j] < n - 1) {
            bounds.push_back(found[2 * j]); bounds.push_back(found[2 * j + 1]);
            last = found[2 * j];
        }
    bounds.push_back(n - 1); bounds.push_back(n - 1);
    const u64 nseg = bounds.size() / 2 - 1;
    HIPCHK(f, hipMemcpyAsync(d_bounds, bounds.data(), bounds.size() * 8, hipMemcpyHostToDevice, f->stream));
    k_fm_walk_samples<<<grid_for(nseg, 256), 256, 0, f->stream>>>(f->V, c->text.as<u64>(), c->sepbits.as<u64>(), d_bounds, nseg,
                                                                  f->sh, f->sa.as<u64>(), counters);
    (void)hipEventRecord(e1, f->stream);
    if (dollar_row % f->s == 0) {                              // the suffix at position 0: no segment's current row
        const u64 zero = 0;
        HIPCHK(f, hipMemcpyAsync(f->sa.as<u64>() + dollar_row / f->s, &zero, 8, hipMemcpyHostToDevice, f->stream));
    }
    u64 ctr[8];
    HIPCHK(f, hipMemcpyAsync(ctr, counters, 64, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;                          // bounds and zero are host memory
    (void)hipEventElapsedTime(&f->ms_samples, e0, e1);
    if (ctr[0] || ctr[1] || ctr[2] || ctr[4] != n - 1) {
        f->err = "the rows are not the BWT of the loaded text (" + std::to_string(ctr[0]) + " symbol mismatches, " +
                 std::to_string(ctr[1]) + " broken links, " + std::to_string(ctr[2]) + " failed searches, " +
                 std::to_string(ctr[4]) + " of " + std::to_string(n - 1) + " steps)";
        return DEBWT_EINVAL;
    }
    return fm_record_starts_build(f);
}

extern "C" int debwt_fm_create(debwt_ctx *c, const uint64_t *rows, const uint64_t *hash_rows, uint64_t dollar_row,
                               uint32_t sa_sample, debwt_fm **out) {
    if (!c || !out) return DEBWT_EINVAL;
    *out = nullptr;
    if (c->stage < ST_LOADED) { c->err = "debwt_fm_create: no text loaded"; return DEBWT_ESTATE; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::vector<u64> hr;
    if (!rows) {                                               // the context's own result
        if (c->stage < ST_ASSEMBLED || c->shard_world > 1) { c->err = "debwt_fm_create: no result of a one-GPU build"; return DEBWT_ESTATE; }
        hr.resize(c->nrec);
        if (c->nrec > 1) HIPCHK(c, hipMemcpy(hr.data(), c->hash_rows.p, (c->nrec - 1) * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&dollar_row, c->dollar.p, 8, hipMemcpyDeviceToHost));
        hr.resize(c->nrec - 1);
    } else {
        if (c->nrec > 1 && !hash_rows) return DEBWT_EINVAL;
        if (c->nrec > 1) hr.assign(hash_rows, hash_rows + (c->nrec - 1));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));               // the index's stream reads the context's text (and rows)
    debwt_fm *f = nullptr;
    int rc = fm_new(c->cfg.device, c->n, c->nrec, sa_sample, &f, &c->err);
    if (rc) return rc;
    rc = fm_create_impl(c, f, rows, hr, dollar_row);
    if (rc) { c->err = f->err; debwt_fm_destroy(f); return rc; }
    *out = f;
    return DEBWT_OK;
}

extern "C" int debwt_fm_open(int device, const uint64_t *rows, uint64_t n, const uint64_t *hash_rows, uint64_t nrec,
                             uint64_t dollar_row, const uint64_t *samples, uint32_t sa_sample, debwt_fm **out) {
    if (!out || !rows || !samples || (nrec > 1 && !hash_rows)) return DEBWT_EINVAL;
    *out = nullptr;
    std::string err;
    debwt_fm *f = nullptr;
    int rc = fm_new(device, n, nrec, sa_sample, &f, &err);
    if (rc) return rc;
    std::vector<u64> hr;
    if (nrec > 1) hr.assign(hash_rows, hash_rows + (nrec - 1));
    {
        FmTmp rows_tmp;
        const u64 *d_words;
        rc = fm_upload_rows(f, rows, &rows_tmp, &d_words);
        if (!rc) rc = fm_build_rank(f, d_words, hr, dollar_row);
    }
    for (u64 i = 0; !rc && i < f->nsamp; i++)
        if (samples[i] >= n) { f->err = "a sample is not a text position"; rc = DEBWT_EINVAL; }
    if (!rc) rc = fm_ensure(f, f->sa, (size_t)f->nsamp * 8);
    if (!rc && hipMemcpy(f->sa.p, samples, (size_t)f->nsamp * 8, hipMemcpyHostToDevice) != hipSuccess) {
        f->err = "upload of the samples"; rc = DEBWT_EDEVICE;
    }
    if (!rc) rc = fm_record_starts_build(f);
    if (rc) { debwt_fm_destroy(f); return rc; }
    *out = f;
    return DEBWT_OK;
}

extern "C" const char *debwt_fm_last_error(const debwt_fm *f) { return f ? f->err.c_str() : ""; }

extern "C" int debwt_fm_info_get(const debwt_fm *f, debwt_fm_info *out) {
    if (!f || !out) return DEBWT_EINVAL;
    memset(out, 0, sizeof *out);
    out->n = f->n; out->nrec = f->nrec; out->sa_sample = f->s; out->samples = f->nsamp;
    out->device_bytes = f->idx.cap + f->rowlists.cap + f->sa.cap + (f->has_text ? f->text.cap : 0) +
                        (f->has_otable ? f->o_table.cap : 0) + (f->has_anchors ? f->anchors.cap : 0) +
                        (f->has_ktable ? f->k_table.cap : 0) + (f->has_ptable ? f->p_table.cap : 0) +
                        (f->has_esa ? f->esa_lcp.cap + f->esa_sa.cap + f->esa_da.cap + f->rec_P.cap : 0);
    out->ms_rank = f->ms_rank; out->ms_samples = f->ms_samples;
    for (int q = 0; q < 4; q++) out->census[q] = f->census[q];
    return DEBWT_OK;
}

extern "C" int debwt_fm_samples(debwt_fm *f, uint64_t *dst, uint64_t capacity) {
    if (!f || !dst) return DEBWT_EINVAL;
    if (capacity < f->nsamp) { f->err = "debwt_fm_samples: capacity below the sample count"; return DEBWT_ERANGE; }
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipMemcpyAsync(dst, f->sa.p, (size_t)f->nsamp * 8, hipMemcpyDeviceToHost, f->stream));
    return fm_sync(f);
}

extern "C" int debwt_fm_record_starts(const debwt_fm *f, uint64_t *dst, uint64_t capacity) {
    if (!f || !dst) return DEBWT_EINVAL;
    if (capacity < f->rec_starts.size()) return DEBWT_ERANGE;
    memcpy(dst, f->rec_starts.data(), f->rec_starts.size() * 8);
    return DEBWT_OK;
}

extern "C" int debwt_fm_count(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat, uint64_t *ranges) {
    if (!f || !offsets || (npat && !ranges)) return DEBWT_EINVAL;
    if (!npat) return DEBWT_OK;
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_count: offsets must not decrease"; return DEBWT_EINVAL; }
    if (offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    HIPCHK(f, hipSetDevice(f->device));
    for (u64 p0 = 0; p0 < npat;) {
        u64 p1 = p0 + 1;                                       // at least one pattern, however long
        while (p1 < npat && p1 - p0 < FM_BATCH_PATTERNS && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS) p1++;
        const u64 np = p1 - p0, base = offsets[p0], bytes = offsets[p1] - base;
        FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(bytes, 1));
        FM_ENSURE(f, f->q_off, (size_t)(np + 1) * 8);
        FM_ENSURE(f, f->q_out, (size_t)np * 16);
        if (bytes) HIPCHK(f, hipMemcpyAsync(f->q_chars.p, patterns + base, bytes, hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->q_off.p, offsets + p0, (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
        k_fm_count<<<grid_for(np, 256), 256, 0, f->stream>>>(f->V, f->q_chars.as<u8>(), f->q_off.as<u64>(), base, np,
                                                             f->q_out.as<u64>());
        HIPCHK(f, hipMemcpyAsync(ranges + 2 * p0, f->q_out.p, np * 16, hipMemcpyDeviceToHost, f->stream));
        int rc = fm_sync(f);                                   // the next batch reuses the scratch
        if (rc) return rc;
        p0 = p1;
    }
    return DEBWT_OK;
}

extern "C" int debwt_fm_locate(debwt_fm *f, const uint64_t *ranges, uint64_t npat, uint64_t max_per_pattern,
                               uint64_t *out_offsets, uint64_t *positions, uint64_t capacity) {
    if (!f || !out_offsets || (npat && !ranges)) return DEBWT_EINVAL;
    out_offsets[0] = 0;
    for (u64 i = 0; i < npat; i++) {
        const u64 lo = ranges[2 * i], hi = ranges[2 * i + 1];
        if (hi < lo || hi > f->n) { f->err = "debwt_fm_locate: a range is not a row interval of the index"; return DEBWT_EINVAL; }
        u64 cnt = hi - lo;
        if (max_per_pattern && cnt > max_per_pattern) cnt = max_per_pattern;
        out_offsets[i + 1] = out_offsets[i] + cnt;
    }
    const u64 total = out_offsets[npat];
    if (!total) return DEBWT_OK;
    if (!positions || capacity < total) { f->err = "debwt_fm_locate: capacity below the reported occurrences"; return DEBWT_ERANGE; }
    HIPCHK(f, hipSetDevice(f->device));
    std::vector<u64> rr, rc_;
    for (u64 p0 = 0; p0 < npat;) {                             // runs uploaded FM_BATCH_PATTERNS patterns at a time
        const u64 p1 = std::min<u64>(npat, p0 + FM_BATCH_PATTERNS);
        rr.clear(); rc_.clear();
        for (u64 i = p0; i < p1; i++)
            if (out_offsets[i + 1] > out_offsets[i]) { rr.push_back(ranges[2 * i]); rc_.push_back(out_offsets[i + 1] - out_offsets[i]); }
        int rc = fm_locate_runs(f, rr, rc_, reinterpret_cast<u64 *>(positions) + out_offsets[p0]);
        if (rc) return rc;
        p0 = p1;
    }
    return DEBWT_OK;
}

// ---- search with mismatches (fm_search_kernels.h) -------------------------------------------------------------------
// Levels are drained depth first: a chunk of level L writes its children into level L + 1's buffer, which is drained
// (recursively) before the next chunk of L, so K + 1 buffers of `cap` items bound the scratch whatever the patterns.
// A chunk whose children or hits exceed a buffer is re-run in a piece sized from the counts it asked for; one item
// asks for at most 4 * 1024 children and one hit, and the buffers hold at least that, so every chunk finishes.

namespace {

constexpr u64 FM_SEARCH_ITEMS = 1ull << 23;            // items per buffer (24 bytes each): 5 buffers = 960 MiB at K = 4

int fm_search_buf(debwt_fm *f, DevBuf &b, size_t bytes) {  // exactly `bytes`: the documented cap is the allocation
    if (bytes <= b.cap) return DEBWT_OK;
    HIPCHK(f, hipStreamSynchronize(f->stream));
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    HIPCHK(f, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return DEBWT_OK;
}

u64 fm_env_u64(const char *name, u64 dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const u64 v = strtoull(e, nullptr, 10);
    return v ? v : dflt;
}

// fn(t, nt) for t = 0 .. nt - 1 on nt host threads: one per 65536 of weight, at most 16 and at most the machine's
template <class Fn>
void fm_host_threads(u64 weight, Fn fn) {
    const unsigned nt = (unsigned)std::max<u64>(1, std::min<u64>({16, std::max(1u, std::thread::hardware_concurrency()), weight / 65536 + 1}));
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back([&fn, t, nt] { fn(t, nt); });
    fn(0, nt);
    for (auto &x : th) x.join();
}

struct FmSearchRun {
    debwt_fm *f;
    const u8 *chars; const u64 *off; u64 base;
    const u32 *plist; u64 nact;
    u32 kmax;
    u64 cap;                                             // items per buffer (children and hits)
    u64 hint[FM_SEARCH_MAX_K + 1];
    hipEvent_t e0, e1;
    std::vector<u64> *hits;                              // (lo, hi, meta) triples
};

int fm_search_drain(FmSearchRun &r, u32 level, u64 count) {
    debwt_fm *f = r.f;
    debwt_fm_search_stats &st = f->s_stats;
    const u64 *in = level ? f->s_items[level].as<u64>() : nullptr;
    u64 *out = level < r.kmax ? f->s_items[level + 1].as<u64>() : nullptr;
    u64 *ctr = f->s_ctr.as<u64>();
    for (u64 a = 0; a < count;) {
        const u64 c = std::min(count - a, r.hint[level]);
        HIPCHK(f, hipMemsetAsync(ctr, 0, 32, f->stream));
        (void)hipEventRecord(r.e0, f->stream);
        k_fm_search<<<grid_for(c, 256), 256, 0, f->stream>>>(f->V, r.chars, r.off, r.base, r.plist, r.nact, in, a, c, level,
                                                             r.kmax, out, out ? r.cap : 0, f->s_hits.as<u64>(), r.cap, ctr);
        (void)hipEventRecord(r.e1, f->stream);
        u64 h[4];
        HIPCHK(f, hipMemcpyAsync(h, ctr, 32, hipMemcpyDeviceToHost, f->stream));
        int rc = fm_sync(f);
        if (rc) return rc;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        st.ms_kernel += ms; st.launches++;
        if (h[0] > r.cap || h[1] > r.cap) {                 // overflow: nothing of this chunk is kept
            if (c == 1) { f->err = "debwt_fm_search: one item overflowed the search buffers"; return DEBWT_EINTERNAL; }
            const double fit = std::min((double)r.cap / (double)std::max<u64>(h[0], 1), (double)r.cap / (double)std::max<u64>(h[1], 1));
            r.hint[level] = std::max<u64>(1, std::min<u64>(c / 2, (u64)((double)c * fit * 0.9)));
            st.retries++;
            continue;
        }
        if (h[1]) {
            const size_t at = r.hits->size();
            r.hits->resize(at + 3 * h[1]);
            HIPCHK(f, hipMemcpyAsync(r.hits->data() + at, f->s_hits.p, h[1] * 24, hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;
        }
        st.items[level] += c; st.steps += h[2]; st.line_reads += h[3];
        if (h[0] < r.cap / 4 && h[1] < r.cap / 4 && r.hint[level] < (1ull << 40)) r.hint[level] *= 2;
        a += c;
        if (h[0] && (rc = fm_search_drain(r, level + 1, h[0]))) return rc;
    }
    return DEBWT_OK;
}

// hits of host patterns [p0, p1) into `hits` as (lo, hi, meta) with global pattern numbers in meta's low 32 bits
// replaced by the offset from p0 (the caller adds p0)
int fm_search_batch(debwt_fm *f, const char *patterns, const uint64_t *offsets, u64 p0, u64 p1, u32 K, u32 flags,
                    u64 cap, std::vector<u64> *hits) {
    const u64 np = p1 - p0, base = offsets[p0], bytes = offsets[p1] - base;
    const u64 nstr = (flags & DEBWT_FM_BOTH_STRANDS) ? 2 : 1;
    FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(bytes, 1));
    FM_ENSURE(f, f->q_off, (size_t)(np + 1) * 8);
    if (bytes) HIPCHK(f, hipMemcpyAsync(f->q_chars.p, patterns + base, bytes, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->q_off.p, offsets + p0, (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
    FmSearchRun r{};
    r.f = f; r.chars = f->q_chars.as<u8>(); r.off = f->q_off.as<u64>(); r.base = base; r.cap = cap; r.hits = hits;
    HIPCHK(f, hipEventCreate(&r.e0));
    if (hipEventCreate(&r.e1) != hipSuccess) { (void)hipEventDestroy(r.e0); f->err = "hipEventCreate"; return DEBWT_EDEVICE; }
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{r.e0, r.e1};
    const bool best = flags & DEBWT_FM_BEST_ONLY;
    std::vector<u32> act;                                  // best only: the patterns without hits yet
    std::vector<u8> found;
    if (best) {
        act.resize(np);
        for (u64 i = 0; i < np; i++) act[i] = (u32)i;
        found.assign(np, 0);
    }
    for (u32 k = best ? 0 : K; k <= K; k++) {              // one stratum, or 0..K over the patterns still without hits
        r.kmax = k;
        for (u32 l = 0; l <= FM_SEARCH_MAX_K; l++) r.hint[l] = ~0ull;
        if (best) {
            if (act.empty()) break;
            FM_ENSURE(f, f->s_plist, act.size() * 4);
            HIPCHK(f, hipMemcpyAsync(f->s_plist.p, act.data(), act.size() * 4, hipMemcpyHostToDevice, f->stream));
            r.plist = f->s_plist.as<u32>(); r.nact = act.size();
        } else {
            r.plist = nullptr; r.nact = np;
        }
        const size_t before = hits->size();
        int rc = fm_search_drain(r, 0, r.nact * nstr);
        if (rc) return rc;
        if (best) {
            for (size_t h = before; h < hits->size(); h += 3) found[(u32)(*hits)[h + 2]] = 1;
            size_t w = 0;
            for (u32 p : act)
                if (!found[p]) act[w++] = p;
            act.resize(w);
        }
    }
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_search(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                               uint32_t max_mismatches, uint32_t flags, uint64_t *hit_offsets, uint64_t *ranges,
                               uint32_t *hit_info, uint64_t capacity) {
    if (!f || !offsets || !hit_offsets) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->s_stats = debwt_fm_search_stats{};
    if (max_mismatches > FM_SEARCH_MAX_K) { f->err = "debwt_fm_search: max_mismatches must be 0..4"; return DEBWT_EINVAL; }
    if (flags & ~(DEBWT_FM_BOTH_STRANDS | DEBWT_FM_BEST_ONLY)) { f->err = "debwt_fm_search: unknown flags"; return DEBWT_EINVAL; }
    if (npat >> 31) { f->err = "debwt_fm_search: too many patterns"; return DEBWT_EINVAL; }
    u64 maxlen = 0;
    for (u64 i = 0; i < npat; i++) {
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_search: offsets must not decrease"; return DEBWT_EINVAL; }
        maxlen = std::max<u64>(maxlen, offsets[i + 1] - offsets[i]);
    }
    if (maxlen > FM_SEARCH_MAX_LEN) {
        f->err = "debwt_fm_search: a pattern is longer than " + std::to_string(FM_SEARCH_MAX_LEN) + " bytes";
        return DEBWT_EINVAL;
    }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    hit_offsets[0] = 0;
    if (!npat) return DEBWT_OK;
    HIPCHK(f, hipSetDevice(f->device));
    // per buffer at least what one item can ask for (4 children per step, 1024 steps), so a chunk of one always fits
    const u64 cap = std::max<u64>(fm_env_u64("DEBWT_FM_SEARCH_ITEMS", FM_SEARCH_ITEMS), 4 * FM_SEARCH_MAX_LEN + 64);
    const u64 batch = std::min<u64>(fm_env_u64("DEBWT_FM_SEARCH_BATCH", FM_BATCH_PATTERNS), FM_BATCH_PATTERNS);
    for (u32 l = 1; l <= max_mismatches; l++) { int rc = fm_search_buf(f, f->s_items[l], (size_t)cap * 24); if (rc) return rc; }
    int rc = fm_search_buf(f, f->s_hits, (size_t)cap * 24);
    if (!rc) rc = fm_search_buf(f, f->s_ctr, 64);
    if (rc) return rc;
    debwt_fm_search_stats &st = f->s_stats;
    st.patterns = npat;
    st.scratch_bytes = (u64)(max_mismatches + 1) * cap * 24;   // the buffers this call may fill
    std::vector<u64> raw;                                  // (lo, hi, meta) with global pattern numbers
    std::vector<u64> part;
    for (u64 p0 = 0; p0 < npat;) {
        u64 p1 = p0 + 1;
        while (p1 < npat && p1 - p0 < batch && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS) p1++;
        part.clear();
        if ((rc = fm_search_batch(f, patterns, offsets, p0, p1, max_mismatches, flags, cap, &part))) return rc;
        for (size_t h = 0; h < part.size(); h += 3) {
            const u64 meta = part[h + 2];
            raw.push_back(part[h]); raw.push_back(part[h + 1]);
            raw.push_back((meta & ~0xFFFFFFFFull) | ((meta & 0xFFFFFFFFull) + p0));
        }
        st.batches++;
        p0 = p1;
    }
    // order: bucket by pattern, then (strand, mismatches, lo) inside each pattern, on up to 16 host threads
    const u64 nh = raw.size() / 3;
    st.hits = nh;
    std::vector<u64> start(npat + 1, 0);
    for (u64 h = 0; h < nh; h++) start[(u32)raw[3 * h + 2] + 1]++;
    for (u64 i = 0; i < npat; i++) start[i + 1] += start[i];
    for (u64 i = 0; i <= npat; i++) hit_offsets[i] = start[i];
    if (capacity < nh || (nh && (!ranges || !hit_info))) {
        f->err = "debwt_fm_search: capacity below the hits (hit_offsets[npat] = " + std::to_string(nh) + ")";
        return DEBWT_ERANGE;
    }
    struct Hit { u64 key, lo, hi; };                       // key: strand << 8 | mismatches (hit_info)
    std::vector<Hit> sorted(nh);
    {
        std::vector<u64> at(start.begin(), start.end() - 1);
        for (u64 h = 0; h < nh; h++) {
            const u64 meta = raw[3 * h + 2];
            sorted[at[(u32)meta]++] = Hit{(((meta >> 56) & 1) << 8) | ((meta >> 48) & 0xFF), raw[3 * h], raw[3 * h + 1]};
        }
    }
    std::vector<u64>().swap(raw);
    fm_host_threads(nh, [&](unsigned t, unsigned nt) {
        for (u64 i = t; i < npat; i += nt)
            std::sort(sorted.begin() + start[i], sorted.begin() + start[i + 1],
                      [](const Hit &x, const Hit &y) { return x.key != y.key ? x.key < y.key : x.lo < y.lo; });
    });
    for (u64 h = 0; h < nh; h++) {
        ranges[2 * h] = sorted[h].lo; ranges[2 * h + 1] = sorted[h].hi;
        hit_info[h] = (u32)sorted[h].key;
    }
    st.ms_wall = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DEBWT_OK;
}

extern "C" int debwt_fm_search_stats_get(const debwt_fm *f, debwt_fm_search_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->s_stats;
    return DEBWT_OK;
}

// ---- maximal exact matches (fm_mem_kernels.h) -----------------------------------------------------------------------
// A batch of patterns [p0, p1) runs as np x strands items; item g gets max(0, m - min_len + 1) slots from an exclusive
// prefix sum (a bound on its MEM count: MEM ends strictly increase and each is >= min_len), so the kernel needs no
// atomics and cannot overflow.  The counts come back, the host lays the MEMs out by (pattern, strand), and
// k_fm_mems_compact gathers them (reversing strand 0, which the lane emits from the right) for one download.

namespace {

constexpr u64 FM_MEM_SLOTS = 1ull << 24;               // worst-case MEM slots per batch (24 bytes each, twice)

struct FmMemOut {                                      // one batch's MEMs, in (pattern, strand, qbeg) order
    std::vector<u64> per;                              // MEMs per (pattern, strand): 2 per pattern
    std::vector<u32> spans;
    std::vector<u64> ranges;
};

int fm_mems_batch(debwt_fm *f, const char *patterns, const uint64_t *offsets, u64 p0, u64 p1, u32 min_len, u64 nstr,
                  hipEvent_t e0, hipEvent_t e1, FmMemOut *out) {
    debwt_fm_mems_stats &st = f->m_stats;
    const u64 np = p1 - p0, base = offsets[p0], bytes = offsets[p1] - base, nit = np * nstr;
    std::vector<u64> slot(nit + 1);
    slot[0] = 0;
    for (u64 g = 0; g < nit; g++) {
        const u64 j = p0 + (g < np ? g : g - np), m = offsets[j + 1] - offsets[j];
        slot[g + 1] = slot[g] + (m >= min_len ? m - min_len + 1 : 0);
    }
    const u64 ns = slot[nit];
    st.scratch_bytes = std::max<u64>(st.scratch_bytes, ns * 24);
    FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(bytes, 1));
    FM_ENSURE(f, f->q_off, (size_t)(np + 1) * 8);
    FM_ENSURE(f, f->m_slot, (size_t)(nit + 1) * 8);
    FM_ENSURE(f, f->m_cnt, (size_t)std::max<u64>(nit, 1) * 4);
    FM_ENSURE(f, f->m_obase, (size_t)std::max<u64>(nit, 1) * 8);
    FM_ENSURE(f, f->m_spans, (size_t)std::max<u64>(ns, 1) * 8);
    FM_ENSURE(f, f->m_ranges, (size_t)std::max<u64>(ns, 1) * 16);
    FM_ENSURE(f, f->s_ctr, 64);
    if (bytes) HIPCHK(f, hipMemcpyAsync(f->q_chars.p, patterns + base, bytes, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->q_off.p, offsets + p0, (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->m_slot.p, slot.data(), (nit + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(f->s_ctr.p, 0, 32, f->stream));
    (void)hipEventRecord(e0, f->stream);
    k_fm_mems<<<grid_for(nit, 256), 256, 0, f->stream>>>(f->V, f->q_chars.as<u8>(), f->q_off.as<u64>(), base, np, nit,
                                                         min_len, f->m_slot.as<u64>(), f->m_spans.as<u32>(),
                                                         f->m_ranges.as<u64>(), f->m_cnt.as<u32>(), f->s_ctr.as<u64>());
    (void)hipEventRecord(e1, f->stream);
    std::vector<u32> cnt(nit);
    u64 h[4];
    HIPCHK(f, hipMemcpyAsync(cnt.data(), f->m_cnt.p, nit * 4, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(h, f->s_ctr.p, 32, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    st.ms_kernel += ms; st.launches++;
    st.steps += h[0]; st.line_reads += h[1]; st.wave_steps += h[2];
    std::vector<u64> ob(nit);                            // output order: pattern, then strand
    out->per.assign(2 * np, 0);
    u64 tot = 0;
    for (u64 j = 0; j < np; j++)
        for (u64 sd = 0; sd < nstr; sd++) {
            const u64 g = sd * np + j;
            if (cnt[g] > slot[g + 1] - slot[g]) { f->err = "debwt_fm_mems: an item wrote more MEMs than its slots"; return DEBWT_EINTERNAL; }
            ob[g] = tot; tot += cnt[g]; out->per[2 * j + sd] = cnt[g];
        }
    out->spans.resize(2 * tot);
    out->ranges.resize(2 * tot);
    if (!tot) return DEBWT_OK;
    FM_ENSURE(f, f->m_cspans, (size_t)tot * 8);
    FM_ENSURE(f, f->m_cranges, (size_t)tot * 16);
    HIPCHK(f, hipMemcpyAsync(f->m_obase.p, ob.data(), nit * 8, hipMemcpyHostToDevice, f->stream));
    k_fm_mems_compact<<<grid_for(nit, 256), 256, 0, f->stream>>>(f->m_slot.as<u64>(), f->m_cnt.as<u32>(),
                                                                 f->m_obase.as<u64>(), np, nit, f->m_spans.as<u32>(),
                                                                 f->m_ranges.as<u64>(), f->m_cspans.as<u32>(),
                                                                 f->m_cranges.as<u64>());
    st.launches++;
    HIPCHK(f, hipMemcpyAsync(out->spans.data(), f->m_cspans.p, tot * 8, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(out->ranges.data(), f->m_cranges.p, tot * 16, hipMemcpyDeviceToHost, f->stream));
    return fm_sync(f);
}

}  // namespace

extern "C" int debwt_fm_mems(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat, uint32_t min_len,
                             uint32_t flags, uint64_t *mem_offsets, uint32_t *spans, uint64_t *ranges, uint8_t *strands,
                             uint64_t capacity) {
    if (!f || !offsets || !mem_offsets) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->m_stats = debwt_fm_mems_stats{};
    if (!min_len) { f->err = "debwt_fm_mems: min_len must be at least 1"; return DEBWT_EINVAL; }
    if (flags & ~DEBWT_FM_BOTH_STRANDS) { f->err = "debwt_fm_mems: unknown flags"; return DEBWT_EINVAL; }
    for (u64 i = 0; i < npat; i++) {
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_mems: offsets must not decrease"; return DEBWT_EINVAL; }
        if ((offsets[i + 1] - offsets[i]) >> 32) { f->err = "debwt_fm_mems: a pattern of 2^32 bytes or more"; return DEBWT_EINVAL; }
    }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    mem_offsets[0] = 0;
    if (!npat) return DEBWT_OK;
    HIPCHK(f, hipSetDevice(f->device));
    const u64 nstr = (flags & DEBWT_FM_BOTH_STRANDS) ? 2 : 1;
    const u64 slots = fm_env_u64("DEBWT_FM_MEM_SLOTS", FM_MEM_SLOTS);
    debwt_fm_mems_stats &st = f->m_stats;
    st.patterns = npat;
    hipEvent_t e0, e1;
    HIPCHK(f, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); f->err = "hipEventCreate"; return DEBWT_EDEVICE; }
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    auto worst = [&](u64 i) {
        const u64 m = offsets[i + 1] - offsets[i];
        return nstr * (m >= min_len ? m - min_len + 1 : 0);
    };
    std::vector<u64> per(2 * npat, 0);                   // MEMs per (pattern, strand)
    std::vector<u32> all_spans;
    std::vector<u64> all_ranges;
    FmMemOut part;
    for (u64 p0 = 0; p0 < npat;) {
        u64 p1 = p0 + 1, ws = worst(p0);                  // at least one pattern, however long
        while (p1 < npat && p1 - p0 < FM_BATCH_PATTERNS && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS &&
               ws + worst(p1) <= slots)
            ws += worst(p1++);
        int rc = fm_mems_batch(f, patterns, offsets, p0, p1, min_len, nstr, e0, e1, &part);
        if (rc) return rc;
        std::copy(part.per.begin(), part.per.end(), per.begin() + 2 * p0);
        all_spans.insert(all_spans.end(), part.spans.begin(), part.spans.end());
        all_ranges.insert(all_ranges.end(), part.ranges.begin(), part.ranges.end());
        st.batches++;
        p0 = p1;
    }
    const u64 total = all_spans.size() / 2;
    st.mems = total;
    for (u64 i = 0; i < npat; i++) mem_offsets[i + 1] = mem_offsets[i] + per[2 * i] + per[2 * i + 1];
    if (capacity < total || (total && (!spans || !ranges || !strands))) {
        f->err = "debwt_fm_mems: capacity below the MEMs (mem_offsets[npat] = " + std::to_string(total) + ")";
        return DEBWT_ERANGE;
    }
    if (total) {
        memcpy(spans, all_spans.data(), total * 8);
        memcpy(ranges, all_ranges.data(), total * 16);
    }
    for (u64 i = 0; i < npat; i++) {
        u8 *d = strands + mem_offsets[i];
        if (per[2 * i]) memset(d, 0, per[2 * i]);
        if (per[2 * i + 1]) memset(d + per[2 * i], 1, per[2 * i + 1]);
    }
    st.ms_wall = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DEBWT_OK;
}

extern "C" int debwt_fm_mems_stats_get(const debwt_fm *f, debwt_fm_mems_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->m_stats;
    return DEBWT_OK;
}

// ---- suffix-prefix overlaps (fm_overlap_kernels.h) ------------------------------------------------------------------
// A batch of patterns [p0, p1) runs as np x strands items with max(0, m - min_overlap + 1) run slots each (one per depth,
// so no atomics and no overflow).  The walk's run and hit counts come back; the host lays runs and hits out by (pattern,
// strand), k_fm_overlap_compact moves the runs there deepest first, and k_fm_overlap_expand writes the hits at most
// DEBWT_FM_OVERLAP_HITS at a launch, straight into the caller's array.  One run is one (pattern, strand, length) group in
// row order; the host sorts every group of two or more by record on up to 16 threads.
// debwt_fm_overlaps and debwt_fm_overlaps_mm share one host path behind their walks: fm_overlaps_call (the batch loop, the
// longest reduction, the capacity protocol) and fm_overlaps_expand, templates over the statistics struct.  Each call
// gives its own two steps: cut and walk the next batch, and put the batch's runs into o_cruns and o_rout.

namespace {

constexpr u64 FM_OVL_SLOTS = 1ull << 24;               // worst-case run slots per batch (16 bytes each)
constexpr u64 FM_OVL_HITS = 1ull << 24;                // hits per expansion launch (16 bytes each)

static_assert(sizeof(debwt_fm_overlap) == sizeof(uint4), "k_fm_overlap_expand writes debwt_fm_overlap as one uint4");

// the record table: for every entry of srows the record that starts at that row, and its length
int fm_overlap_table(debwt_fm *f) {
    if (f->has_otable) return DEBWT_OK;
    const u64 nrec = f->nrec, n = f->n;
    if (nrec >> 32) { f->err = "debwt_fm_overlaps: 2^32 records or more"; return DEBWT_EINVAL; }
    std::vector<u64> sr(nrec), pos(nrec - 1);
    HIPCHK(f, hipMemcpyAsync(sr.data(), f->V.srows, nrec * 8, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    if (nrec > 1 && (rc = fm_locate_runs(f, {f->V.C[4]}, {nrec - 1}, pos.data()))) return rc;   // LF of the j-th '#' row
    const std::vector<u64> &rs = f->rec_starts;
    std::vector<FmOvlRec> tab(nrec);
    u64 jh = 0, dollars = 0;
    for (u64 k = 0; k < nrec; k++) {
        u64 rec = 0;
        if (sr[k] == f->dollar_row) dollars++;
        else if (jh < nrec - 1) {
            const u64 p = pos[jh++] + 1;
            rec = (u64)(std::lower_bound(rs.begin(), rs.end(), p) - rs.begin());
            if (rec == 0 || rec >= nrec || rs[rec] != p) {
                f->err = "debwt_fm_overlaps: a '#' row does not lead to a record start"; return DEBWT_EINTERNAL;
            }
        } else dollars = 2;                                    // more '#' rows than records: reported below
        const u64 len = (rec + 1 < nrec ? rs[rec + 1] - 1 : n - 1) - rs[rec];
        tab[k] = FmOvlRec{(u32)rec, (u32)std::min<u64>(len, 0xFFFFFFFFull)};
    }
    if (dollars != 1 || jh != nrec - 1) { f->err = "debwt_fm_overlaps: the separator rows are inconsistent"; return DEBWT_EINTERNAL; }
    FM_ENSURE(f, f->o_table, (size_t)nrec * sizeof(FmOvlRec));
    HIPCHK(f, hipMemcpyAsync(f->o_table.p, tab.data(), nrec * sizeof(FmOvlRec), hipMemcpyHostToDevice, f->stream));
    if ((rc = fm_sync(f))) return rc;                          // tab is host memory
    f->has_otable = true;
    return DEBWT_OK;
}

struct FmOvlBatch {
    u64 p0 = 0, np = 0, nruns = 0, nhits = 0;
    std::vector<u64> per;                                  // hits per pattern of the batch
    u64 nit = 0;                                           // the exact walk's: items, their slots, first run and first hit
    std::vector<u64> slot, rbase, hbase;
    std::vector<uint4> raw;                                // the mismatch walk's: runs as the levels wrote them,
    std::vector<FmOvlRun> cruns;                           // ordered in k_fm_overlap_expand's layout,
    std::vector<u64> rout;                                 // and the first hit number of each
};

// the walk of one batch: fills b (run and hit layout in (pattern, strand) order) and the counters
int fm_overlaps_walk(debwt_fm *f, const char *patterns, const uint64_t *offsets, u64 p0, u64 p1, u32 min_overlap, u64 nstr,
                     hipEvent_t e0, hipEvent_t e1, FmOvlBatch *b) {
    debwt_fm_overlaps_stats &st = f->o_stats;
    const u64 np = p1 - p0, base = offsets[p0], bytes = offsets[p1] - base, nit = np * nstr;
    b->p0 = p0; b->np = np; b->nit = nit;
    b->slot.resize(nit + 1);
    b->slot[0] = 0;
    for (u64 g = 0; g < nit; g++) {
        const u64 j = p0 + (g < np ? g : g - np), m = offsets[j + 1] - offsets[j];
        b->slot[g + 1] = b->slot[g] + (m >= min_overlap ? m - min_overlap + 1 : 0);
    }
    const u64 ns = b->slot[nit];
    FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(bytes, 1));
    FM_ENSURE(f, f->q_off, (size_t)(np + 1) * 8);
    FM_ENSURE(f, f->o_slot, (size_t)(nit + 1) * 8);
    FM_ENSURE(f, f->o_nruns, (size_t)nit * 4);
    FM_ENSURE(f, f->o_nhits, (size_t)nit * 8);
    FM_ENSURE(f, f->o_runs, (size_t)std::max<u64>(ns, 1) * sizeof(FmOvlRun));
    FM_ENSURE(f, f->s_ctr, 64);
    if (bytes) HIPCHK(f, hipMemcpyAsync(f->q_chars.p, patterns + base, bytes, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->q_off.p, offsets + p0, (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->o_slot.p, b->slot.data(), (nit + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(f->s_ctr.p, 0, 32, f->stream));
    (void)hipEventRecord(e0, f->stream);
    k_fm_overlap_walk<<<grid_for(nit, 256), 256, 0, f->stream>>>(f->V, f->q_chars.as<u8>(), f->q_off.as<u64>(), base, np, nit,
                                                                 min_overlap, f->o_slot.as<u64>(), f->o_runs.as<FmOvlRun>(),
                                                                 f->o_nruns.as<u32>(), f->o_nhits.as<u64>(), f->s_ctr.as<u64>());
    (void)hipEventRecord(e1, f->stream);
    std::vector<u32> nr(nit);
    std::vector<u64> nh(nit);
    u64 h[4];
    HIPCHK(f, hipMemcpyAsync(nr.data(), f->o_nruns.p, nit * 4, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(nh.data(), f->o_nhits.p, nit * 8, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(h, f->s_ctr.p, 32, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    st.ms_kernel += ms; st.launches++;
    st.steps += h[0]; st.line_reads += h[1]; st.wave_steps += h[2];
    b->rbase.resize(nit); b->hbase.resize(nit); b->per.assign(np, 0);
    u64 tr = 0, th = 0;
    for (u64 j = 0; j < np; j++)
        for (u64 sd = 0; sd < nstr; sd++) {
            const u64 g = sd * np + j;
            if (nr[g] > b->slot[g + 1] - b->slot[g]) { f->err = "debwt_fm_overlaps: an item wrote more runs than its slots"; return DEBWT_EINTERNAL; }
            b->rbase[g] = tr; b->hbase[g] = th;
            tr += nr[g]; th += nh[g]; b->per[j] += nh[g];
        }
    b->nruns = tr; b->nhits = th;
    st.runs += tr;
    st.scratch_bytes = std::max<u64>(st.scratch_bytes, ns * sizeof(FmOvlRun) + nit * 36 + tr * 24);
    return DEBWT_OK;
}

// the exact call's runs step: the walked batch's runs from their slots to o_cruns, with o_rout.  ev.a is recorded in
// front of the compaction, so the first expansion launch is timed together with it.
int fm_overlaps_compact(debwt_fm *f, const FmOvlBatch &b, u64 chunk, FmEvents &ev) {
    debwt_fm_overlaps_stats &st = f->o_stats;
    FM_ENSURE(f, f->o_rbase, (size_t)b.nit * 8);
    FM_ENSURE(f, f->o_hbase, (size_t)b.nit * 8);
    st.scratch_bytes = std::max<u64>(st.scratch_bytes, b.slot[b.nit] * sizeof(FmOvlRun) + b.nit * 36 + b.nruns * 24 + chunk * 16);
    HIPCHK(f, hipMemcpyAsync(f->o_rbase.p, b.rbase.data(), b.nit * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->o_hbase.p, b.hbase.data(), b.nit * 8, hipMemcpyHostToDevice, f->stream));
    (void)hipEventRecord(ev.a, f->stream);
    k_fm_overlap_compact<<<grid_for(b.nit, 256), 256, 0, f->stream>>>(f->q_off.as<u64>(), f->o_slot.as<u64>(), f->o_nruns.as<u32>(),
                                                                      f->o_rbase.as<u64>(), f->o_hbase.as<u64>(), b.np, b.nit,
                                                                      f->o_runs.as<FmOvlRun>(), f->o_cruns.as<FmOvlRun>(),
                                                                      f->o_rout.as<u64>());
    st.launches++;
    return DEBWT_OK;
}

// The hits of a walked batch into dst (b.nhits of them), in the documented order.  runs(f, b, chunk, ev) fills o_cruns
// and o_rout, which are reserved here, and records ev.a behind its uploads: the first launch is timed from there.
template <class St, class Runs>
int fm_overlaps_expand(debwt_fm *f, St &st, const FmOvlBatch &b, u64 limit, FmEvents &ev, Runs &runs, debwt_fm_overlap *dst) {
    if (!b.nhits) return DEBWT_OK;
    const u64 chunk = std::min(b.nhits, limit);
    FM_ENSURE(f, f->o_cruns, (size_t)b.nruns * sizeof(FmOvlRun));
    FM_ENSURE(f, f->o_rout, (size_t)b.nruns * 8);
    FM_ENSURE(f, f->o_hits, (size_t)chunk * sizeof(uint4));
    if (int rc = runs(f, b, chunk, ev)) return rc;
    for (u64 g0 = 0; g0 < b.nhits; g0 += chunk) {
        const u64 cnt = std::min(b.nhits - g0, chunk);
        if (g0) (void)hipEventRecord(ev.a, f->stream);
        k_fm_overlap_expand<<<grid_for(cnt, 256), 256, 0, f->stream>>>(f->o_cruns.as<FmOvlRun>(), f->o_rout.as<u64>(), b.nruns,
                                                                       f->o_table.as<FmOvlRec>(), g0, cnt, f->o_hits.as<uint4>());
        (void)hipEventRecord(ev.b, f->stream);
        HIPCHK(f, hipMemcpyAsync(dst + g0, f->o_hits.p, cnt * sizeof(uint4), hipMemcpyDeviceToHost, f->stream));
        if (int rc = fm_sync(f)) return rc;                    // the next launch reuses o_hits
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev.a, ev.b);
        st.ms_kernel += ms; st.launches++;
    }
    // record order inside every (pattern, strand, length) group, whatever runs it is made of
    std::vector<u64> start(b.np + 1, 0);
    for (u64 j = 0; j < b.np; j++) start[j + 1] = start[j] + b.per[j];
    fm_host_threads(b.nhits, [&](unsigned t, unsigned nt) {
        for (u64 j = t; j < b.np; j += nt)
            for (u64 a = start[j]; a < start[j + 1];) {
                u64 e = a + 1;
                while (e < start[j + 1] && dst[e].strand == dst[a].strand && dst[e].length == dst[a].length) e++;
                if (e - a > 1)
                    std::sort(dst + a, dst + e, [](const debwt_fm_overlap &x, const debwt_fm_overlap &y) { return x.record < y.record; });
                a = e;
            }
    });
    return DEBWT_OK;
}

// What both calls do behind their argument checks.  walk(p0, ev, &b) cuts the batch that starts at pattern p0 and walks
// it; runs as in fm_overlaps_expand.  Once the hits so far exceed the capacity the batches are only counted.
template <class St, class Walk, class Runs>
int fm_overlaps_call(debwt_fm *f, St &st, const char *who, std::chrono::steady_clock::time_point t0, u64 npat, u32 flags,
                     uint64_t *hit_offsets, debwt_fm_overlap *hits, u64 capacity, Walk walk, Runs runs) {
    const bool longest = (flags & DEBWT_FM_OVERLAP_LONGEST) != 0;
    const u64 limit = fm_env_u64("DEBWT_FM_OVERLAP_HITS", FM_OVL_HITS);
    st.patterns = npat;
    FmEvents ev;
    int rc = ev.init(f);
    if (rc) return rc;
    FmOvlBatch b;
    std::vector<debwt_fm_overlap> tmp;                     // DEBWT_FM_OVERLAP_LONGEST: a batch's hits before the reduction
    std::vector<uint64_t> loc;
    bool fits = true;                                      // false once the hits so far exceed the capacity: count only
    for (u64 p0 = 0; p0 < npat; p0 += b.np) {
        if ((rc = walk(p0, ev, &b))) return rc;
        const u64 at = hit_offsets[p0];
        if (longest) {
            tmp.resize(b.nhits);
            if ((rc = fm_overlaps_expand(f, st, b, limit, ev, runs, tmp.data()))) return rc;
            loc.assign(b.np + 1, 0);
            for (u64 j = 0; j < b.np; j++) loc[j + 1] = loc[j] + b.per[j];
            if ((rc = debwt_fm_overlap_longest(tmp.data(), loc.data(), b.np, loc.data()))) {
                f->err = std::string(who) + ": a batch's hits are not in order"; return DEBWT_EINTERNAL;
            }
            for (u64 j = 0; j < b.np; j++) hit_offsets[p0 + j + 1] = at + loc[j + 1];
            fits = fits && hits && at + loc[b.np] <= capacity;   // a NULL array never fits here, even for no hits
            if (fits && loc[b.np]) memcpy(hits + at, tmp.data(), loc[b.np] * sizeof(debwt_fm_overlap));
        } else {
            for (u64 j = 0; j < b.np; j++) hit_offsets[p0 + j + 1] = hit_offsets[p0 + j] + b.per[j];
            fits = fits && (hits || !b.nhits) && at + b.nhits <= capacity;
            if (fits && (rc = fm_overlaps_expand(f, st, b, limit, ev, runs, hits + at))) return rc;
        }
        st.batches++;
    }
    const u64 total = hit_offsets[npat];
    st.hits = total;
    if (!fits || capacity < total) {
        f->err = std::string(who) + ": capacity below the hits (hit_offsets[npat] = " + std::to_string(total) + ")";
        return DEBWT_ERANGE;
    }
    st.ms_wall = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_overlap_longest(debwt_fm_overlap *hits, const uint64_t *offsets_in, uint64_t npat, uint64_t *offsets_out) {
    if (!offsets_in || !offsets_out || (npat && offsets_in[npat] > offsets_in[0] && !hits)) return DEBWT_EINVAL;
    for (u64 i = 0; i < npat; i++) {                           // the whole input is checked before anything moves
        if (offsets_in[i + 1] < offsets_in[i]) return DEBWT_EINVAL;
        for (u64 h = offsets_in[i]; h < offsets_in[i + 1]; h++) {
            const debwt_fm_overlap &x = hits[h];
            if (x.strand > 1) return DEBWT_EINVAL;
            if (h == offsets_in[i]) continue;
            const debwt_fm_overlap &w = hits[h - 1];
            if (x.strand != w.strand ? x.strand < w.strand
                                     : x.length != w.length ? x.length > w.length : x.record <= w.record) return DEBWT_EINVAL;
        }
    }
    u64 out = npat ? offsets_in[0] : 0;
    std::vector<std::pair<u32, u64>> by;                   // (record, hit) of one pattern and strand
    std::vector<u8> keep;
    for (u64 i = 0; i < npat; i++) {
        const u64 a = offsets_in[i], e = offsets_in[i + 1];
        offsets_out[i] = out;
        for (u64 s = a; s < e;) {
            u64 t = s + 1;
            while (t < e && hits[t].strand == hits[s].strand) t++;
            if (t - s <= 64) {                                 // the usual case: against the hits kept so far, which lie
                const u64 o0 = out;                            // at or before h and hold every record's first hit
                for (u64 h = s; h < t; h++) {
                    u64 g = o0;
                    while (g < out && hits[g].record != hits[h].record) g++;
                    if (g == out) hits[out++] = hits[h];
                }
                s = t;
                continue;
            }
            by.clear();
            for (u64 h = s; h < t; h++) by.emplace_back(hits[h].record, h);
            std::sort(by.begin(), by.end());                 // per record the earliest hit first: its largest length
            keep.assign(t - s, 0);
            for (size_t k = 0; k < by.size(); k++)
                if (!k || by[k].first != by[k - 1].first) keep[by[k].second - s] = 1;
            for (u64 h = s; h < t; h++)
                if (keep[h - s]) hits[out++] = hits[h];
            s = t;
        }
    }
    offsets_out[npat] = out;
    return DEBWT_OK;
}

extern "C" int debwt_fm_overlaps(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                                 uint32_t min_overlap, uint32_t flags, uint64_t *hit_offsets, debwt_fm_overlap *hits,
                                 uint64_t capacity) {
    if (!f || !offsets || !hit_offsets) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->o_stats = debwt_fm_overlaps_stats{};
    if (!min_overlap) { f->err = "debwt_fm_overlaps: min_overlap must be at least 1"; return DEBWT_EINVAL; }
    if (flags & ~(DEBWT_FM_BOTH_STRANDS | DEBWT_FM_OVERLAP_LONGEST)) { f->err = "debwt_fm_overlaps: unknown flags"; return DEBWT_EINVAL; }
    u64 maxlen = 0;
    for (u64 i = 0; i < npat; i++) {
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_overlaps: offsets must not decrease"; return DEBWT_EINVAL; }
        if ((offsets[i + 1] - offsets[i]) >> 32) { f->err = "debwt_fm_overlaps: a pattern of 2^32 bytes or more"; return DEBWT_EINVAL; }
        maxlen = std::max<u64>(maxlen, offsets[i + 1] - offsets[i]);
    }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    hit_offsets[0] = 0;
    if (!npat) return DEBWT_OK;
    HIPCHK(f, hipSetDevice(f->device));
    int rc = fm_overlap_table(f);
    if (rc) return rc;
    const u64 nstr = (flags & DEBWT_FM_BOTH_STRANDS) ? 2 : 1;
    const u64 slots = fm_env_u64("DEBWT_FM_OVERLAP_SLOTS", FM_OVL_SLOTS);
    auto worst = [&](u64 i) {
        const u64 m = offsets[i + 1] - offsets[i];
        return nstr * (m >= min_overlap ? m - min_overlap + 1 : 0);
    };
    auto walk = [&](u64 p0, FmEvents &ev, FmOvlBatch *b) {
        u64 p1 = p0 + 1, ws = worst(p0);                  // at least one pattern, however long
        while (p1 < npat && p1 - p0 < FM_BATCH_PATTERNS && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS &&
               ws + worst(p1) <= slots)
            ws += worst(p1++);
        return fm_overlaps_walk(f, patterns, offsets, p0, p1, min_overlap, nstr, ev.a, ev.b, b);
    };
    if ((rc = fm_overlaps_call(f, f->o_stats, "debwt_fm_overlaps", t0, npat, flags, hit_offsets, hits, capacity, walk,
                               fm_overlaps_compact)))
        return rc;
    if (maxlen == 0xFFFFFFFFull)                           // the table's lengths stop at 2^32 - 1: such overlaps from the starts
        for (u64 h = 0; h < hit_offsets[npat]; h++)
            if (hits[h].length == 0xFFFFFFFFu) {
                const u64 r = hits[h].record;
                const u64 len = (r + 1 < f->nrec ? f->rec_starts[r + 1] - 1 : f->n - 1) - f->rec_starts[r];
                hits[h].flags = (hits[h].flags & ~DEBWT_FM_OVERLAP_CONTAINS) | (len == 0xFFFFFFFFull ? DEBWT_FM_OVERLAP_CONTAINS : 0u);
            }
    return DEBWT_OK;
}

extern "C" int debwt_fm_overlaps_stats_get(const debwt_fm *f, debwt_fm_overlaps_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->o_stats;
    return DEBWT_OK;
}

// ---- suffix-prefix overlaps with mismatches (fm_overlap_mm_kernels.h) -----------------------------------------------
// The levels of a batch are drained depth first as in debwt_fm_search: a chunk of level L writes its children into level
// L + 1's buffer, which is drained before the next chunk of L, and its runs into the run buffer, which comes back to the
// host after every chunk.  One item asks for at most 4 * 1024 children and 1024 + 1 runs, and the buffers hold at least
// that, so every chunk finishes.  The host orders the batch's runs by (pattern, strand, length descending, first entry),
// which gives the exact hit counts, and uploads them with their first hit numbers in place of the exact call's compaction;
// from there on the path is the exact call's (fm_overlaps_call, fm_overlaps_expand, k_fm_overlap_expand).  A (pattern,
// strand, length) group may be made of several runs (one per work item), so its hits are sorted by record as a whole.

namespace {

constexpr u64 FM_OVL_MM_ITEMS = 1ull << 23;            // entries per buffer: 24 bytes an item, 16 a run

struct FmOvlMmRun {
    debwt_fm *f;
    const u8 *chars; const u64 *off; u64 base, np;
    u32 kmax, min_overlap, permille;
    u64 cap;                                             // entries per buffer (children and runs)
    u64 hint[FM_SEARCH_MAX_K + 1];
    hipEvent_t e0, e1;
    std::vector<uint4> *runs;                            // (batch-local pattern, first entry, entries, d | level << 16 | strand << 24)
};

int fm_overlap_mm_drain(FmOvlMmRun &r, u32 level, u64 count) {
    debwt_fm *f = r.f;
    debwt_fm_overlaps_mm_stats &st = f->om_stats;
    const u64 *in = level ? f->s_items[level].as<u64>() : nullptr;
    u64 *out = level < r.kmax ? f->s_items[level + 1].as<u64>() : nullptr;
    u64 *ctr = f->s_ctr.as<u64>();
    for (u64 a = 0; a < count;) {
        const u64 c = std::min(count - a, r.hint[level]);
        HIPCHK(f, hipMemsetAsync(ctr, 0, 40, f->stream));
        (void)hipEventRecord(r.e0, f->stream);
        k_fm_overlap_mm<<<grid_for(c, 256), 256, 0, f->stream>>>(f->V, r.chars, r.off, r.base, r.np, in, a, c, level, r.kmax,
                                                                 r.min_overlap, r.permille, out, out ? r.cap : 0,
                                                                 f->s_hits.as<uint4>(), r.cap, ctr);
        (void)hipEventRecord(r.e1, f->stream);
        u64 h[5];
        HIPCHK(f, hipMemcpyAsync(h, ctr, 40, hipMemcpyDeviceToHost, f->stream));
        int rc = fm_sync(f);
        if (rc) return rc;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        st.ms_kernel += ms; st.launches++;
        if (h[0] > r.cap || h[1] > r.cap) {                 // overflow: nothing of this chunk is kept
            if (c == 1) { f->err = "debwt_fm_overlaps_mm: one item overflowed the buffers"; return DEBWT_EINTERNAL; }
            const double fit = std::min((double)r.cap / (double)std::max<u64>(h[0], 1), (double)r.cap / (double)std::max<u64>(h[1], 1));
            r.hint[level] = std::max<u64>(1, std::min<u64>(c / 2, (u64)((double)c * fit * 0.9)));
            st.retries++;
            continue;
        }
        if (h[1]) {
            const size_t at = r.runs->size();
            r.runs->resize(at + h[1]);
            HIPCHK(f, hipMemcpyAsync(r.runs->data() + at, f->s_hits.p, h[1] * sizeof(uint4), hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;
        }
        st.items[level] += c; st.steps += h[2]; st.line_reads += h[3]; st.wave_steps += h[4];
        if (h[0] < r.cap / 4 && h[1] < r.cap / 4 && r.hint[level] < (1ull << 40)) r.hint[level] *= 2;
        a += c;
        if (h[0] && (rc = fm_overlap_mm_drain(r, level + 1, h[0]))) return rc;
    }
    return DEBWT_OK;
}

// the levels of one batch, then its runs in order: fills b
int fm_overlaps_mm_walk(debwt_fm *f, const char *patterns, const uint64_t *offsets, u64 p0, u64 p1, u64 nstr, FmOvlMmRun &r,
                        FmOvlBatch *b) {
    debwt_fm_overlaps_mm_stats &st = f->om_stats;
    const u64 np = p1 - p0, base = offsets[p0], bytes = offsets[p1] - base;
    b->p0 = p0; b->np = np;
    b->raw.clear();
    FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(bytes, 1));
    FM_ENSURE(f, f->q_off, (size_t)(np + 1) * 8);
    if (bytes) HIPCHK(f, hipMemcpyAsync(f->q_chars.p, patterns + base, bytes, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->q_off.p, offsets + p0, (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
    r.chars = f->q_chars.as<u8>(); r.off = f->q_off.as<u64>(); r.base = base; r.np = np; r.runs = &b->raw;
    int rc = fm_overlap_mm_drain(r, 0, np * nstr);
    if (rc) return rc;
    const u64 nr = b->raw.size();
    // bucket by pattern, then (strand, length descending, first entry) inside each pattern, on up to 16 host threads
    std::vector<u64> start(np + 1, 0);
    for (u64 k = 0; k < nr; k++) {
        if (b->raw[k].x >= np) { f->err = "debwt_fm_overlaps_mm: a run names a pattern outside its batch"; return DEBWT_EINTERNAL; }
        start[b->raw[k].x + 1]++;
    }
    for (u64 j = 0; j < np; j++) start[j + 1] += start[j];
    b->cruns.resize(nr); b->rout.resize(nr); b->per.assign(np, 0);
    {
        std::vector<u64> at(start.begin(), start.end() - 1);
        for (u64 k = 0; k < nr; k++) b->cruns[at[b->raw[k].x]++] = b->raw[k];
    }
    fm_host_threads(nr, [&](unsigned t, unsigned nt) {
        for (u64 j = t; j < np; j += nt) {
            const u32 m = (u32)(offsets[p0 + j + 1] - offsets[p0 + j]);
            FmOvlRun *a = b->cruns.data() + start[j], *e = b->cruns.data() + start[j + 1];
            std::sort(a, e, [](const FmOvlRun &x, const FmOvlRun &y) {
                const u32 sx = x.w >> 24, sy = y.w >> 24, dx = x.w & 0xFFFFu, dy = y.w & 0xFFFFu;
                return sx != sy ? sx < sy : dx != dy ? dx > dy : x.y < y.y;
            });
            u64 h = 0;
            for (FmOvlRun *x = a; x < e; x++) {              // to the expansion's layout
                const u32 d = x->w & 0xFFFFu, lv = (x->w >> 16) & 0xFFu, sd = x->w >> 24;
                h += x->z;
                *x = make_uint4(d, x->y, x->z, sd | (d == m ? 2u : 0u) | (lv << 8));
            }
            b->per[j] = h;
        }
    });
    u64 h = 0;
    for (u64 k = 0; k < nr; k++) { b->rout[k] = h; h += b->cruns[k].z; }
    b->nruns = nr; b->nhits = h;
    st.runs += nr;
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_overlaps_mm(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                                    uint32_t min_overlap, uint32_t max_mismatches, uint32_t max_error_permille, uint32_t flags,
                                    uint64_t *hit_offsets, debwt_fm_overlap *hits, uint64_t capacity) {
    if (!f || !offsets || !hit_offsets) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->om_stats = debwt_fm_overlaps_mm_stats{};
    if (!min_overlap) { f->err = "debwt_fm_overlaps_mm: min_overlap must be at least 1"; return DEBWT_EINVAL; }
    if (max_mismatches > FM_SEARCH_MAX_K) { f->err = "debwt_fm_overlaps_mm: max_mismatches must be 0..4"; return DEBWT_EINVAL; }
    if (max_error_permille > 1000) { f->err = "debwt_fm_overlaps_mm: max_error_permille must be 0..1000"; return DEBWT_EINVAL; }
    if (flags & ~(DEBWT_FM_BOTH_STRANDS | DEBWT_FM_OVERLAP_LONGEST)) { f->err = "debwt_fm_overlaps_mm: unknown flags"; return DEBWT_EINVAL; }
    if (npat >> 31) { f->err = "debwt_fm_overlaps_mm: too many patterns"; return DEBWT_EINVAL; }
    for (u64 i = 0; i < npat; i++) {
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_overlaps_mm: offsets must not decrease"; return DEBWT_EINVAL; }
        if (offsets[i + 1] - offsets[i] > FM_SEARCH_MAX_LEN) {
            f->err = "debwt_fm_overlaps_mm: a pattern is longer than " + std::to_string(FM_SEARCH_MAX_LEN) + " bytes";
            return DEBWT_EINVAL;
        }
    }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    hit_offsets[0] = 0;
    if (!npat) return DEBWT_OK;
    HIPCHK(f, hipSetDevice(f->device));
    int rc = fm_overlap_table(f);
    if (rc) return rc;
    const u64 nstr = (flags & DEBWT_FM_BOTH_STRANDS) ? 2 : 1;
    // per buffer at least what one item can ask for (4 children per step, 1024 steps; a run per step and one on arrival)
    const u64 cap = std::max<u64>(fm_env_u64("DEBWT_FM_OVERLAP_ITEMS", FM_OVL_MM_ITEMS), 4 * FM_SEARCH_MAX_LEN + 64);
    const u64 batch = std::min<u64>(fm_env_u64("DEBWT_FM_OVERLAP_BATCH", FM_BATCH_PATTERNS), FM_BATCH_PATTERNS);
    for (u32 l = 1; l <= max_mismatches; l++) if ((rc = fm_search_buf(f, f->s_items[l], (size_t)cap * 24))) return rc;
    if ((rc = fm_search_buf(f, f->s_hits, (size_t)cap * sizeof(uint4)))) return rc;
    if ((rc = fm_search_buf(f, f->s_ctr, 64))) return rc;
    debwt_fm_overlaps_mm_stats &st = f->om_stats;
    const u64 fixed = (u64)max_mismatches * cap * 24 + cap * sizeof(uint4);   // the level and run buffers this call may fill
    st.scratch_bytes = fixed;
    FmOvlMmRun r{};
    r.f = f; r.kmax = max_mismatches; r.min_overlap = min_overlap; r.permille = max_error_permille; r.cap = cap;
    for (u32 l = 0; l <= FM_SEARCH_MAX_K; l++) r.hint[l] = ~0ull;
    auto walk = [&](u64 p0, FmEvents &ev, FmOvlBatch *b) {
        u64 p1 = p0 + 1;
        while (p1 < npat && p1 - p0 < batch && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS) p1++;
        r.e0 = ev.a; r.e1 = ev.b;
        return fm_overlaps_mm_walk(f, patterns, offsets, p0, p1, nstr, r, b);
    };
    auto runs = [&](debwt_fm *f, const FmOvlBatch &b, u64 chunk, FmEvents &ev) -> int {
        st.scratch_bytes = std::max<u64>(st.scratch_bytes, fixed + b.nruns * 24 + chunk * 16);
        HIPCHK(f, hipMemcpyAsync(f->o_cruns.p, b.cruns.data(), b.nruns * sizeof(FmOvlRun), hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->o_rout.p, b.rout.data(), b.nruns * 8, hipMemcpyHostToDevice, f->stream));
        (void)hipEventRecord(ev.a, f->stream);
        return DEBWT_OK;
    };
    return fm_overlaps_call(f, st, "debwt_fm_overlaps_mm", t0, npat, flags, hit_offsets, hits, capacity, walk, runs);
}

extern "C" int debwt_fm_overlaps_mm_stats_get(const debwt_fm *f, debwt_fm_overlaps_mm_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->om_stats;
    return DEBWT_OK;
}

// ---- gapped extension of seeds and the read mapper (fm_extend_kernels.h) --------------------------------------------
// Jobs whose band misses their record never reach the device.  The others run in batches cut at DEBWT_FM_EXTEND_BYTES of
// traceback flags: the sweep (a group of 16, 32 or 64 lanes per job, by the band), then with a traceback the walk twice
// with one lane per job -- once to count the CIGAR ops, once to write them at their final offsets.

namespace {

constexpr u64 FM_EXTEND_BYTES = 512ull << 20;          // flag scratch per batch
constexpr u64 FM_EXTEND_JOBS = 1ull << 20;             // jobs per batch
constexpr u32 FM_EXT_LDS_BUDGET = 64u << 10;           // staged queries and text windows of one workgroup

// the device form of a job; false: no cell of the band lies inside the record (score 0)
bool fm_ext_prepare(const debwt_fm *f, u64 m, const debwt_fm_job &jb, u32 w, FmExtJob *d) {
    const u64 rs = f->rec_starts[jb.record];
    const u64 re = (jb.record + 1 < f->nrec ? f->rec_starts[jb.record + 1] : f->n) - 1;
    const __int128 tb = (__int128)jb.diag - (__int128)w;   // text position of band column 0
    const __int128 ncol = (__int128)m + 2 * w;
    __int128 lo = (__int128)rs - tb, hi = (__int128)re - tb;
    if (lo < 0) lo = 0;
    if (hi > ncol) hi = ncol;
    if (lo >= hi) return false;
    const u32 clo = (u32)lo, chi = (u32)hi;
    const u32 ilo = clo > 2 * w ? clo - 2 * w : 0, ihi = (u32)std::min<u64>(m, chi);
    d->tbase = (long long)tb;
    d->m = (u32)m; d->strand = jb.strand; d->clo = clo; d->chi = chi;
    d->a0 = 2 * ilo; d->nsteps = 2 * (ihi - 1) + 2 * w - d->a0 + 1;
    d->qoff = 0; d->flag_off = 0;
    return true;
}

template <int G>
void fm_ext_launch(bool trace, u32 grid, u32 block, size_t lds, hipStream_t s, const u64 *text, const u8 *chars,
                   const FmExtJob *jobs, u32 nj, u32 w, const debwt_fm_scoring &sc, u32 lds_per_job, u8 *flags, u64 *best,
                   u32 *cells) {
    if (trace)
        k_fm_extend<G, true><<<grid, block, lds, s>>>(text, chars, jobs, nj, w, sc.match, sc.mismatch, sc.gap_open,
                                                      sc.gap_extend, lds_per_job, flags, best, cells);
    else
        k_fm_extend<G, false><<<grid, block, lds, s>>>(text, chars, jobs, nj, w, sc.match, sc.mismatch, sc.gap_open,
                                                       sc.gap_extend, lds_per_job, flags, best, cells);
}

// jobs [0, njobs) -> out; with `trace` also ops per job (cig_n) and the ops of all jobs in job order (cig).  The
// arguments were validated by the caller; statistics are added to f->x_stats.
int fm_extend_run(debwt_fm *f, const char *patterns, const uint64_t *offsets, const debwt_fm_job *jobs, u64 njobs,
                  const debwt_fm_scoring &sc, u32 w, bool trace, debwt_fm_aln *out, std::vector<u32> *cig_n,
                  std::vector<u32> *cig) {
    debwt_fm_extend_stats &st = f->x_stats;
    st.jobs += njobs;
    if (trace) { cig_n->assign(njobs, 0); cig->clear(); }
    if (!njobs) return DEBWT_OK;
    const u64 limit = fm_env_u64("DEBWT_FM_EXTEND_BYTES", FM_EXTEND_BYTES);
    const int G = w < 16 ? 16 : w < 32 ? 32 : 64;
    FmEvents ev;
    if (int rc = ev.init(f)) return rc;
    std::vector<FmExtJob> dj;
    std::vector<u64> src;                                // job index of every device job
    std::vector<char> chars;
    std::vector<u64> best;
    std::vector<u32> cells, tr, ops;
    std::vector<u64> coff;
    for (u64 j0 = 0; j0 < njobs;) {
        dj.clear(); src.clear(); chars.clear();
        u64 fbytes = 0, j1 = j0, last_pat = ~0ull, last_off = 0;
        u32 lds_job = 4;
        for (; j1 < njobs; j1++) {
            const debwt_fm_job &jb = jobs[j1];
            const u64 m = offsets[jb.pattern + 1] - offsets[jb.pattern];
            FmExtJob d;
            if (!fm_ext_prepare(f, m, jb, w, &d)) { out[j1] = debwt_fm_aln{}; continue; }
            const u64 fb = trace ? (u64)d.nsteps * (w + 1) : 0;
            const bool fresh = jb.pattern != last_pat;
            if (!dj.empty() && (fbytes + fb > limit || dj.size() >= FM_EXTEND_JOBS ||
                                (fresh && chars.size() + m > FM_BATCH_CHARS)))
                break;
            if (fresh) {
                last_pat = jb.pattern; last_off = chars.size();
                chars.insert(chars.end(), patterns + offsets[jb.pattern], patterns + offsets[jb.pattern] + m);
            }
            d.qoff = last_off; d.flag_off = fbytes;
            fbytes += fb;
            lds_job = std::max<u32>(lds_job, (u32)(((m + 1) / 2 + (m + 2 * w + 3) / 4 + 3) & ~3ull));
            dj.push_back(d); src.push_back(j1);
        }
        const u64 nd = dj.size();
        if (!nd) { j0 = j1; continue; }
        // the workgroup: as many groups as the staged strings of its jobs leave room for
        int g = G;
        u32 block = 256;
        if ((u64)(block / g) * lds_job > FM_EXT_LDS_BUDGET) block = 64;
        while ((u64)(block / g) * lds_job > FM_EXT_LDS_BUDGET && g < 64) g *= 2;
        const u32 jpb = block / g, grid = (u32)((nd + jpb - 1) / jpb);
        const u32 jpw = 64 / g;                            // wave steps: the longest job of every wave
        for (u64 a = 0; a < nd; a += jpw) {
            u32 mx = 0;
            for (u64 b = a; b < std::min(nd, a + jpw); b++) mx = std::max(mx, (dj[b].nsteps + 1) & ~1u);
            st.wave_steps += mx;
        }
        st.scratch_bytes = std::max<u64>(st.scratch_bytes, fbytes);
        FM_ENSURE(f, f->q_chars, std::max<size_t>(chars.size(), 1));
        FM_ENSURE(f, f->x_jobs, nd * sizeof(FmExtJob));
        FM_ENSURE(f, f->x_best, nd * 8);
        FM_ENSURE(f, f->x_cells, nd * 4);
        if (trace) {
            FM_ENSURE(f, f->x_flags, (size_t)std::max<u64>(fbytes, 1));
            FM_ENSURE(f, f->x_tr, nd * 16);
            FM_ENSURE(f, f->x_cigoff, (nd + 1) * 8);
        }
        HIPCHK(f, hipMemcpyAsync(f->q_chars.p, chars.data(), chars.size(), hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->x_jobs.p, dj.data(), nd * sizeof(FmExtJob), hipMemcpyHostToDevice, f->stream));
        (void)hipEventRecord(ev.a, f->stream);
        const size_t lds = (size_t)jpb * lds_job;
        auto go = [&](auto tag) {
            fm_ext_launch<decltype(tag)::value>(trace, grid, block, lds, f->stream, f->text.as<u64>(), f->q_chars.as<u8>(),
                                                f->x_jobs.as<FmExtJob>(), (u32)nd, w, sc, lds_job, f->x_flags.as<u8>(),
                                                f->x_best.as<u64>(), f->x_cells.as<u32>());
        };
        if (g == 16) go(std::integral_constant<int, 16>{});
        else if (g == 32) go(std::integral_constant<int, 32>{});
        else go(std::integral_constant<int, 64>{});
        (void)hipEventRecord(ev.b, f->stream);
        st.launches++;
        best.resize(nd); cells.resize(nd);
        HIPCHK(f, hipMemcpyAsync(best.data(), f->x_best.p, nd * 8, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(f, hipMemcpyAsync(cells.data(), f->x_cells.p, nd * 4, hipMemcpyDeviceToHost, f->stream));
        if (trace) {
            k_fm_extend_trace<<<grid_for(nd, 256), 256, 0, f->stream>>>(f->x_jobs.as<FmExtJob>(), (u32)nd, w, f->x_flags.as<u8>(),
                                                                        f->x_best.as<u64>(), nullptr, nullptr, f->x_tr.as<u32>());
            st.launches++;
            tr.resize(4 * nd);
            HIPCHK(f, hipMemcpyAsync(tr.data(), f->x_tr.p, nd * 16, hipMemcpyDeviceToHost, f->stream));
        }
        int rc = fm_sync(f);
        if (rc) return rc;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev.a, ev.b);
        st.ms_kernel += ms;
        for (u64 a = 0; a < nd; a++) st.cells += cells[a];
        u64 total = 0;
        if (trace) {
            coff.resize(nd + 1);
            coff[0] = 0;
            for (u64 a = 0; a < nd; a++) coff[a + 1] = coff[a] + tr[4 * a + 3];
            total = coff[nd];
            ops.resize(total);
            if (total) {
                FM_ENSURE(f, f->x_cig, (size_t)total * 4);
                HIPCHK(f, hipMemcpyAsync(f->x_cigoff.p, coff.data(), (nd + 1) * 8, hipMemcpyHostToDevice, f->stream));
                (void)hipEventRecord(ev.a, f->stream);
                k_fm_extend_trace<<<grid_for(nd, 256), 256, 0, f->stream>>>(f->x_jobs.as<FmExtJob>(), (u32)nd, w,
                                                                            f->x_flags.as<u8>(), f->x_best.as<u64>(),
                                                                            f->x_cigoff.as<u64>(), f->x_cig.as<u32>(),
                                                                            f->x_tr.as<u32>());
                (void)hipEventRecord(ev.b, f->stream);
                st.launches++;
                HIPCHK(f, hipMemcpyAsync(ops.data(), f->x_cig.p, total * 4, hipMemcpyDeviceToHost, f->stream));
                if ((rc = fm_sync(f))) return rc;
                (void)hipEventElapsedTime(&ms, ev.a, ev.b);
                st.ms_trace += ms;
            }
        }
        for (u64 a = 0; a < nd; a++) {
            debwt_fm_aln &o = out[src[a]];
            o = debwt_fm_aln{};
            const u64 key = best[a];
            if (!(key >> 32)) continue;
            const u32 i = 65535u - (u32)((key >> 8) & 0xFFFFu), k = 127u - (u32)(key & 0xFFu);
            o.score = (int32_t)(key >> 32);
            o.qend = i + 1;
            o.tend = (u64)(dj[a].tbase + (long long)(i + k)) + 1;
            if (trace) {
                o.qbeg = tr[4 * a]; o.tbeg = (u64)(dj[a].tbase + (long long)tr[4 * a + 1]); o.edits = tr[4 * a + 2];
                (*cig_n)[src[a]] = tr[4 * a + 3];
            }
        }
        if (trace) cig->insert(cig->end(), ops.begin(), ops.end());   // device jobs are in job order
        st.batches++;
        j0 = j1;
    }
    return DEBWT_OK;
}

int fm_ext_check(debwt_fm *f, const debwt_fm_scoring *sc, u32 band, const char *who) {
    if (!f->has_text) { f->err = std::string(who) + ": no text attached (debwt_fm_attach_text)"; return DEBWT_ESTATE; }
    if (band > FM_EXT_MAX_BAND) { f->err = std::string(who) + ": band above 63"; return DEBWT_EINVAL; }
    if (sc->match < 1 || sc->match > 255 || sc->mismatch < 1 || sc->mismatch > 255 || sc->gap_open < 0 || sc->gap_open > 255 ||
        sc->gap_extend < 1 || sc->gap_extend > 255) {
        f->err = std::string(who) + ": scoring outside match 1..255, mismatch 1..255, gap open 0..255, gap extend 1..255";
        return DEBWT_EINVAL;
    }
    return DEBWT_OK;
}

double fm_ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" int debwt_fm_attach_text(debwt_fm *f, debwt_ctx *c, const uint64_t *packed, const uint64_t *sep) {
    if (!f) return DEBWT_EINVAL;
    const u64 n = f->n, nrec = f->nrec;
    if (c) {
        if (c->stage < ST_LOADED) { f->err = "debwt_fm_attach_text: the context holds no text"; return DEBWT_ESTATE; }
        if (c->n != n || c->nrec != nrec) { f->err = "debwt_fm_attach_text: the context's text has another n or nrec"; return DEBWT_EINVAL; }
        sep = c->h_sep.data();
    } else if (!packed || !sep) return DEBWT_EINVAL;
    for (u64 r = 0; r < nrec; r++) {
        const u64 want = (r + 1 < nrec ? f->rec_starts[r + 1] : n) - 1;
        if (sep[r] != want) {
            f->err = "debwt_fm_attach_text: separator " + std::to_string(r) + " is at " + std::to_string(sep[r]) +
                     ", the index has it at " + std::to_string(want);
            return DEBWT_EINVAL;
        }
    }
    HIPCHK(f, hipSetDevice(f->device));
    f->has_text = false;
    const size_t words = (size_t)((n + 63) >> 5), tw = words + 2;
    FM_ENSURE(f, f->text, tw * 8);
    FM_ENSURE(f, f->s_ctr, 64);
    if (c) {
        HIPCHK(f, hipStreamSynchronize(c->stream));          // the load may still be in flight on the context's stream
        HIPCHK(f, hipMemcpyAsync(f->text.p, c->text.p, words * 8, hipMemcpyDeviceToDevice, f->stream));
    } else {
        HIPCHK(f, hipMemcpyAsync(f->text.p, packed, words * 8, hipMemcpyHostToDevice, f->stream));
    }
    HIPCHK(f, hipMemsetAsync(f->text.as<u64>() + words, 0, (tw - words) * 8, f->stream));
    HIPCHK(f, hipMemsetAsync(f->s_ctr.p, 0, 8, f->stream));
    k_fm_text_check<<<grid_for(f->nsamp, 256), 256, 0, f->stream>>>(f->V, f->sa.as<u64>(), f->nsamp, f->sh, f->text.as<u64>(),
                                                                   f->s_ctr.as<u64>());
    u64 bad = 0;
    HIPCHK(f, hipMemcpyAsync(&bad, f->s_ctr.p, 8, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    if (bad) {
        f->err = "debwt_fm_attach_text: not the text of the index (" + std::to_string(bad) + " of " + std::to_string(f->nsamp) +
                 " sampled rows hold another symbol than the text before their suffix)";
        return DEBWT_EINVAL;
    }
    f->has_text = true;
    return DEBWT_OK;
}

extern "C" int debwt_fm_extend(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                               const debwt_fm_job *jobs, uint64_t njobs, const debwt_fm_scoring *sc, uint32_t band,
                               debwt_fm_aln *out, uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity) {
    if (!f || !sc || !offsets || (njobs && (!jobs || !out))) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->x_stats = debwt_fm_extend_stats{};
    int rc = fm_ext_check(f, sc, band, "debwt_fm_extend");
    if (rc) return rc;
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_extend: offsets must not decrease"; return DEBWT_EINVAL; }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    for (u64 j = 0; j < njobs; j++) {
        const debwt_fm_job &jb = jobs[j];
        if (jb.pattern >= npat || jb.strand > 1 || jb.record >= f->nrec) {
            f->err = "debwt_fm_extend: job " + std::to_string(j) + " names a pattern, strand or record that does not exist";
            return DEBWT_EINVAL;
        }
        const u64 m = offsets[jb.pattern + 1] - offsets[jb.pattern];
        if (m < 1 || m > FM_EXT_MAX_LEN) {
            f->err = "debwt_fm_extend: job " + std::to_string(j) + " has a pattern of " + std::to_string(m) + " bytes (1..65535)";
            return DEBWT_EINVAL;
        }
    }
    HIPCHK(f, hipSetDevice(f->device));
    const bool trace = cigar_offsets != nullptr;
    std::vector<u32> cig_n, cig;
    rc = fm_extend_run(f, patterns, offsets, jobs, njobs, *sc, band, trace, out, &cig_n, &cig);
    if (rc) return rc;
    f->x_stats.ms_wall = (float)fm_ms_since(t0);
    if (!trace) return DEBWT_OK;
    cigar_offsets[0] = 0;
    for (u64 j = 0; j < njobs; j++) cigar_offsets[j + 1] = cigar_offsets[j] + cig_n[j];
    if (capacity < cig.size() || (!cig.empty() && !cigar)) {
        f->err = "debwt_fm_extend: capacity below the CIGAR ops (cigar_offsets[njobs] = " + std::to_string(cig.size()) + ")";
        return DEBWT_ERANGE;
    }
    if (!cig.empty()) memcpy(cigar, cig.data(), cig.size() * 4);
    return DEBWT_OK;
}

extern "C" int debwt_fm_extend_stats_get(const debwt_fm *f, debwt_fm_extend_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->x_stats;
    return DEBWT_OK;
}

extern "C" int debwt_fm_cluster_seeds(const debwt_fm_seed *seeds, uint64_t nseeds, uint32_t band, uint32_t max_cand,
                                      debwt_fm_cand *out) {
    if ((nseeds && !seeds) || (max_cand && !out)) return DEBWT_EINVAL;
    for (u64 i = 0; i < nseeds; i++)
        if (seeds[i].qend <= seeds[i].qbeg) return DEBWT_EINVAL;
    std::vector<u64> ord(nseeds);
    for (u64 i = 0; i < nseeds; i++) ord[i] = i;
    auto key = [&](u64 i) { return std::make_tuple(seeds[i].strand, seeds[i].record, seeds[i].diag, seeds[i].qbeg, seeds[i].qend); };
    std::sort(ord.begin(), ord.end(), [&](u64 a, u64 b) { return key(a) < key(b); });
    std::vector<debwt_fm_cand> cl;
    std::vector<std::pair<u32, u32>> iv;
    auto close = [&](debwt_fm_cand &c) {                   // weight: the union of the cluster's query intervals
        std::sort(iv.begin(), iv.end());
        u32 end = 0, wgt = 0;
        for (auto &p : iv) {
            const u32 a = std::max(p.first, end);
            if (p.second > a) { wgt += p.second - a; end = p.second; }
        }
        c.weight = wgt;
        iv.clear();
    };
    u32 best_len = 0, best_qbeg = 0;
    for (u64 x = 0; x < nseeds; x++) {
        const debwt_fm_seed &s = seeds[ord[x]];
        const bool join = !cl.empty() && cl.back().strand == s.strand && cl.back().record == s.record &&
                          (__int128)s.diag - (__int128)cl.back().first_diag <= (__int128)band;
        if (!join) {
            if (!cl.empty()) close(cl.back());
            cl.push_back(debwt_fm_cand{s.diag, s.diag, s.record, s.strand, 0, 0});
            best_len = 0;
        }
        debwt_fm_cand &c = cl.back();
        c.seeds++;
        iv.emplace_back(s.qbeg, s.qend);
        const u32 len = s.qend - s.qbeg;
        if (len > best_len || (len == best_len && s.qbeg < best_qbeg)) { best_len = len; best_qbeg = s.qbeg; c.diag = s.diag; }
    }
    if (!cl.empty()) close(cl.back());
    std::stable_sort(cl.begin(), cl.end(), [](const debwt_fm_cand &a, const debwt_fm_cand &b) {
        if (a.weight != b.weight) return a.weight > b.weight;
        return std::make_tuple(a.strand, a.record, a.first_diag) < std::make_tuple(b.strand, b.record, b.first_diag);
    });
    const u64 k = std::min<u64>(cl.size(), max_cand);
    for (u64 i = 0; i < k; i++) out[i] = cl[i];
    return (int)k;
}

extern "C" void debwt_fm_map_defaults(debwt_fm_map_opts *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->min_len = 19; o->band = 16; o->max_occ = 64; o->max_cand = 8; o->min_score = 30; o->flags = 0;
    o->scoring = debwt_fm_scoring{1, 4, 6, 1};
}

extern "C" int debwt_fm_map(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                            const debwt_fm_map_opts *opts, debwt_fm_hit *hits, uint64_t *cigar_offsets, uint32_t *cigar,
                            uint64_t capacity) {
    if (!f || !offsets || !cigar_offsets || (npat && !hits)) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    debwt_fm_map_opts o;
    debwt_fm_map_defaults(&o);
    if (opts) o = *opts;
    f->map_stats = debwt_fm_map_stats{};
    f->x_stats = debwt_fm_extend_stats{};
    int rc = fm_ext_check(f, &o.scoring, o.band, "debwt_fm_map");
    if (rc) return rc;
    if (!o.min_len || !o.max_occ || !o.max_cand || o.max_cand > 4096 || (o.flags & ~DEBWT_FM_MAP_FORWARD)) {
        f->err = "debwt_fm_map: min_len, max_occ and max_cand must be positive (max_cand <= 4096), flags known";
        return DEBWT_EINVAL;
    }
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_map: offsets must not decrease"; return DEBWT_EINVAL; }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    debwt_fm_map_stats &ms = f->map_stats;
    ms.reads = npat;
    cigar_offsets[0] = 0;
    std::vector<u32> all_cig;
    std::vector<uint64_t> moff, ranges, loff, pos;
    std::vector<u32> spans, cig_n, cig;
    std::vector<u8> strands;
    std::vector<debwt_fm_seed> seeds;
    std::vector<debwt_fm_cand> cand(o.max_cand);
    std::vector<debwt_fm_job> jobs;
    std::vector<u64> job_first;
    std::vector<debwt_fm_aln> aln;
    const u32 mflags = (o.flags & DEBWT_FM_MAP_FORWARD) ? 0u : DEBWT_FM_BOTH_STRANDS;
    for (u64 p0 = 0; p0 < npat;) {
        u64 p1 = p0 + 1;
        while (p1 < npat && p1 - p0 < (1ull << 18) && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS) p1++;
        const u64 np = p1 - p0;
        // 1. MEMs of the batch (the existing path, as any caller uses it)
        auto t = std::chrono::steady_clock::now();
        moff.assign(np + 1, 0);
        u64 cap = std::max<u64>(spans.size() / 2, 4 * np + 16);
        for (;;) {
            spans.resize(2 * cap); ranges.resize(2 * cap); strands.resize(cap);
            rc = debwt_fm_mems(f, patterns, offsets + p0, np, o.min_len, mflags, moff.data(), spans.data(), ranges.data(),
                               strands.data(), cap);
            if (rc == DEBWT_ERANGE && moff[np] > cap) { cap = moff[np]; continue; }
            if (rc) return rc;
            break;
        }
        const u64 nmem = moff[np];
        ms.mems += nmem;
        ms.ms_mems += (float)fm_ms_since(t);
        // 2. their first max_occ rows located
        t = std::chrono::steady_clock::now();
        loff.assign(nmem + 1, 0);
        u64 nocc = 0;
        for (u64 i = 0; i < nmem; i++) nocc += std::min<u64>(ranges[2 * i + 1] - ranges[2 * i], o.max_occ);
        pos.resize(std::max<u64>(nocc, 1));
        rc = debwt_fm_locate(f, ranges.data(), nmem, o.max_occ, loff.data(), pos.data(), pos.size());
        if (rc) return rc;
        ms.seeds += nocc;
        ms.ms_locate += (float)fm_ms_since(t);
        // 3. seeds -> candidates -> jobs, read by read
        t = std::chrono::steady_clock::now();
        jobs.clear();
        job_first.assign(np + 1, 0);
        for (u64 r = 0; r < np; r++) {
            job_first[r] = jobs.size();
            const u64 m = offsets[p0 + r + 1] - offsets[p0 + r];
            if (m < 1 || m > FM_EXT_MAX_LEN) continue;
            seeds.clear();
            for (u64 i = moff[r]; i < moff[r + 1]; i++) {
                const u32 qb = strands[i] ? (u32)m - spans[2 * i + 1] : spans[2 * i];      // in Q
                const u32 qe = strands[i] ? (u32)m - spans[2 * i] : spans[2 * i + 1];
                for (u64 x = loff[i]; x < loff[i + 1]; x++) {
                    const u64 tp = pos[x];
                    const u64 rec = (u64)(std::upper_bound(f->rec_starts.begin(), f->rec_starts.end(), tp) - f->rec_starts.begin()) - 1;
                    seeds.push_back(debwt_fm_seed{(int64_t)tp - (int64_t)qb, (u32)rec, strands[i], qb, qe});
                }
            }
            if (seeds.empty()) continue;
            const int nc = debwt_fm_cluster_seeds(seeds.data(), seeds.size(), o.band, o.max_cand, cand.data());
            if (nc < 0) { f->err = "debwt_fm_map: a MEM with an empty span"; return DEBWT_EINTERNAL; }
            for (int k = 0; k < nc; k++) jobs.push_back(debwt_fm_job{p0 + r, cand[k].diag, cand[k].record, cand[k].strand});
        }
        job_first[np] = jobs.size();
        ms.candidates += jobs.size();
        ms.jobs += jobs.size();
        ms.ms_candidates += (float)fm_ms_since(t);
        // 4. every job extended, with its traceback: the tie rule and `sub` need the text interval of each
        t = std::chrono::steady_clock::now();
        aln.resize(jobs.size());
        HIPCHK(f, hipSetDevice(f->device));
        rc = fm_extend_run(f, patterns, offsets, jobs.data(), jobs.size(), o.scoring, o.band, true, aln.data(), &cig_n, &cig);
        if (rc) return rc;
        ms.ms_extend += (float)fm_ms_since(t);
        // 5. the winner of every read
        std::vector<u64> cfirst(jobs.size() + 1, 0);
        for (u64 j = 0; j < jobs.size(); j++) cfirst[j + 1] = cfirst[j] + cig_n[j];
        for (u64 r = 0; r < np; r++) {
            const u64 m = offsets[p0 + r + 1] - offsets[p0 + r];
            debwt_fm_hit &h = hits[p0 + r];
            memset(&h, 0, sizeof h);
            h.pattern = p0 + r;
            h.flags = DEBWT_FM_MAP_UNMAPPED | (m > FM_EXT_MAX_LEN ? DEBWT_FM_MAP_TOO_LONG : 0u);
            cigar_offsets[p0 + r + 1] = cigar_offsets[p0 + r];
            u64 w = ~0ull;
            for (u64 j = job_first[r]; j < job_first[r + 1]; j++) {
                if (aln[j].score <= 0) continue;
                if (w == ~0ull || aln[j].score > aln[w].score ||
                    (aln[j].score == aln[w].score && std::make_tuple(jobs[j].strand, jobs[j].record, aln[j].tbeg) <
                                                         std::make_tuple(jobs[w].strand, jobs[w].record, aln[w].tbeg)))
                    w = j;
            }
            if (w == ~0ull || aln[w].score < o.min_score) continue;
            int32_t sub = 0;
            for (u64 j = job_first[r]; j < job_first[r + 1]; j++)
                if (j != w && aln[j].score > sub && (aln[j].tend <= aln[w].tbeg || aln[j].tbeg >= aln[w].tend)) sub = aln[j].score;
            const debwt_fm_aln &a = aln[w];
            h.flags = jobs[w].strand ? DEBWT_FM_MAP_REVERSE : 0u;
            h.record = jobs[w].record; h.offset = a.tbeg - f->rec_starts[jobs[w].record];
            h.qbeg = a.qbeg; h.qend = a.qend; h.tbeg = a.tbeg; h.tend = a.tend;
            h.score = a.score; h.sub = sub; h.mapq = (u32)(60 * (int64_t)(a.score - sub) / a.score); h.edits = a.edits;
            h.diag = jobs[w].diag;
            all_cig.insert(all_cig.end(), cig.begin() + cfirst[w], cig.begin() + cfirst[w + 1]);
            cigar_offsets[p0 + r + 1] = all_cig.size();
            ms.mapped++;
        }
        ms.batches++;
        p0 = p1;
    }
    f->x_stats.ms_wall = ms.ms_extend;
    ms.ms_wall = (float)fm_ms_since(t0);
    if (capacity < all_cig.size() || (!all_cig.empty() && !cigar)) {
        f->err = "debwt_fm_map: capacity below the CIGAR ops (cigar_offsets[npat] = " + std::to_string(all_cig.size()) + ")";
        return DEBWT_ERANGE;
    }
    if (!all_cig.empty()) memcpy(cigar, all_cig.data(), all_cig.size() * 4);
    return DEBWT_OK;
}

extern "C" int debwt_fm_map_stats_get(const debwt_fm *f, debwt_fm_map_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->map_stats;
    return DEBWT_OK;
}

// ---- chains: seeds of a read chained across diagonals, extension along a chain, the mapper on both (fm_chain_kernels.h) --
// The batches, the two traceback passes and the statistics are those of fm_extend_run; a job carries its anchors, and its
// flag scratch is one row of 2w + 1 bytes per query row that holds an allowed cell.

namespace {

// the device form of a chain job; false: no cell of the band lies inside the record (score 0)
bool fm_chain_prepare(const debwt_fm *f, u64 m, const debwt_fm_chain_job &jb, const debwt_fm_anchor *an, u32 w, FmChainJob *d) {
    const u64 rs = f->rec_starts[jb.record];
    const u64 re = (jb.record + 1 < f->nrec ? f->rec_starts[jb.record + 1] : f->n) - 1;
    const __int128 tb = (__int128)an[0].diag - (__int128)w;   // text position of column 0
    const __int128 lim = (__int128)1 << 30;                   // columns of allowed cells stay far inside it
    const long long clo = (long long)std::max(-lim, std::min(lim, (__int128)rs - tb));
    const long long chi = (long long)std::max(-lim, std::min(lim, (__int128)re - tb));
    long long i0 = -1, i1 = -1, wmin = 0, wmax = 0;
    u32 a0 = 0;
    for (u32 a = 0; a < jb.n_anchors; a++) {                  // the rows [ra, rb) share the centre of anchor a
        const long long ra = a ? (long long)an[a].qbeg : 0, rb = a + 1 < jb.n_anchors ? (long long)an[a + 1].qbeg : (long long)m;
        const long long dc = (long long)(an[a].diag - an[0].diag);
        const long long lo = std::max(ra, clo - dc - 2 * (long long)w), hi = std::min(rb - 1, chi - 1 - dc);
        if (lo > hi) continue;
        const long long c0 = std::max(clo, lo + dc), c1 = std::min(chi - 1, hi + dc + 2 * (long long)w);
        if (i0 < 0) { i0 = lo; a0 = a; wmin = c0; wmax = c1; }
        i1 = hi + 1;
        wmin = std::min(wmin, c0); wmax = std::max(wmax, c1);
    }
    if (i0 < 0) return false;
    d->tbase = (long long)tb;
    d->m = (u32)m; d->strand = jb.strand; d->na = jb.n_anchors; d->a0 = a0;
    d->clo = (int)clo; d->chi = (int)chi;
    d->wlo = (int)wmin; d->wn = (u32)(wmax - wmin + 1);
    d->i0 = (u32)i0; d->nrows = (u32)(i1 - i0);
    d->qoff = 0; d->flag_off = 0; d->aoff = 0;
    return true;
}

template <int G, int S>
void fm_chain_launch(bool trace, u32 grid, u32 block, size_t lds, hipStream_t s, const u64 *text, const u8 *chars,
                     const FmChainJob *jobs, const FmChainAnchor *anchors, u32 nj, u32 w, const debwt_fm_scoring &sc,
                     u32 lds_per_job, u8 *flags, u64 *best, u32 *cells) {
    if (trace)
        k_fm_extend_chain<G, S, true><<<grid, block, lds, s>>>(text, chars, jobs, anchors, nj, w, sc.match, sc.mismatch,
                                                               sc.gap_open, sc.gap_extend, lds_per_job, flags, best, cells);
    else
        k_fm_extend_chain<G, S, false><<<grid, block, lds, s>>>(text, chars, jobs, anchors, nj, w, sc.match, sc.mismatch,
                                                                sc.gap_open, sc.gap_extend, lds_per_job, flags, best, cells);
}

// chain jobs [0, njobs) -> out; with `trace` also ops per job (cig_n) and the ops of all jobs in job order (cig).  The
// arguments were validated by the caller; statistics are added to f->x_stats (wave steps: rows).
int fm_chain_run(debwt_fm *f, const char *patterns, const uint64_t *offsets, const debwt_fm_chain_job *jobs, u64 njobs,
                 const debwt_fm_anchor *anchors, const debwt_fm_scoring &sc, u32 w, bool trace, debwt_fm_aln *out,
                 std::vector<u32> *cig_n, std::vector<u32> *cig) {
    debwt_fm_extend_stats &st = f->x_stats;
    st.jobs += njobs;
    if (trace) { cig_n->assign(njobs, 0); cig->clear(); }
    if (!njobs) return DEBWT_OK;
    const u64 limit = fm_env_u64("DEBWT_FM_EXTEND_BYTES", FM_EXTEND_BYTES);
    const int G = 2 * w + 1 <= 16 ? 16 : 2 * w + 1 <= 32 ? 32 : 64;
    FmEvents ev;
    if (int rc = ev.init(f)) return rc;
    std::vector<FmChainJob> dj;
    std::vector<FmChainAnchor> da;
    std::vector<u64> src;                                // job index of every device job
    std::vector<char> chars;
    std::vector<u64> best;
    std::vector<u32> cells, tr, ops;
    std::vector<u64> coff;
    for (u64 j0 = 0; j0 < njobs;) {
        dj.clear(); da.clear(); src.clear(); chars.clear();
        u64 fbytes = 0, j1 = j0, last_pat = ~0ull, last_off = 0;
        u32 lds_job = 4;
        for (; j1 < njobs; j1++) {
            const debwt_fm_chain_job &jb = jobs[j1];
            const debwt_fm_anchor *an = anchors + jb.first_anchor;
            const u64 m = offsets[jb.pattern + 1] - offsets[jb.pattern];
            FmChainJob d;
            if (!fm_chain_prepare(f, m, jb, an, w, &d)) { out[j1] = debwt_fm_aln{}; continue; }
            const u64 fb = trace ? (u64)d.nrows * (2 * w + 1) : 0;
            const bool fresh = jb.pattern != last_pat;
            if (!dj.empty() && (fbytes + fb > limit || dj.size() >= FM_EXTEND_JOBS ||
                                (fresh && chars.size() + m > FM_BATCH_CHARS)))
                break;
            if (fresh) {
                last_pat = jb.pattern; last_off = chars.size();
                chars.insert(chars.end(), patterns + offsets[jb.pattern], patterns + offsets[jb.pattern] + m);
            }
            d.qoff = last_off; d.flag_off = fbytes; d.aoff = da.size();
            fbytes += fb;
            for (u32 a = 0; a < jb.n_anchors; a++) da.push_back(FmChainAnchor{an[a].qbeg, (int)(an[a].diag - an[0].diag)});
            // a text window that leaves no room beside the query is not staged: the sweep reads the text itself
            if ((m + 1) / 2 + ((u64)d.wn + 3) / 4 + 3 > FM_EXT_LDS_BUDGET) d.wn = 0;
            lds_job = std::max<u32>(lds_job, (u32)(((m + 1) / 2 + ((u64)d.wn + 3) / 4 + 3) & ~3ull));
            dj.push_back(d); src.push_back(j1);
        }
        const u64 nd = dj.size();
        if (!nd) { j0 = j1; continue; }
        // the workgroup: as many groups as the staged strings of its jobs leave room for
        int g = G;
        u32 block = 256;
        if ((u64)(block / g) * lds_job > FM_EXT_LDS_BUDGET) block = 64;
        while ((u64)(block / g) * lds_job > FM_EXT_LDS_BUDGET && g < 64) g *= 2;
        const u32 jpb = block / g, grid = (u32)((nd + jpb - 1) / jpb);
        const u32 jpw = 64 / g;                            // wave steps: the rows of the longest job of every wave
        for (u64 a = 0; a < nd; a += jpw) {
            u32 mx = 0;
            for (u64 b = a; b < std::min(nd, a + jpw); b++) mx = std::max(mx, dj[b].nrows);
            st.wave_steps += mx;
        }
        st.scratch_bytes = std::max<u64>(st.scratch_bytes, fbytes);
        FM_ENSURE(f, f->q_chars, std::max<size_t>(chars.size(), 1));
        FM_ENSURE(f, f->x_jobs, nd * sizeof(FmChainJob));
        FM_ENSURE(f, f->x_anchors, da.size() * sizeof(FmChainAnchor));
        FM_ENSURE(f, f->x_best, nd * 8);
        FM_ENSURE(f, f->x_cells, nd * 4);
        if (trace) {
            FM_ENSURE(f, f->x_flags, (size_t)std::max<u64>(fbytes, 1));
            FM_ENSURE(f, f->x_tr, nd * 16);
            FM_ENSURE(f, f->x_cigoff, (nd + 1) * 8);
        }
        HIPCHK(f, hipMemcpyAsync(f->q_chars.p, chars.data(), chars.size(), hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->x_jobs.p, dj.data(), nd * sizeof(FmChainJob), hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->x_anchors.p, da.data(), da.size() * sizeof(FmChainAnchor), hipMemcpyHostToDevice, f->stream));
        (void)hipEventRecord(ev.a, f->stream);
        const size_t lds = (size_t)jpb * lds_job;
        auto go = [&](auto gt, auto stag) {
            fm_chain_launch<decltype(gt)::value, decltype(stag)::value>(
                trace, grid, block, lds, f->stream, f->text.as<u64>(), f->q_chars.as<u8>(), f->x_jobs.as<FmChainJob>(),
                f->x_anchors.as<FmChainAnchor>(), (u32)nd, w, sc, lds_job, f->x_flags.as<u8>(), f->x_best.as<u64>(),
                f->x_cells.as<u32>());
        };
        if (w > 31) go(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
        else if (g == 16) go(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{});
        else if (g == 32) go(std::integral_constant<int, 32>{}, std::integral_constant<int, 1>{});
        else go(std::integral_constant<int, 64>{}, std::integral_constant<int, 1>{});
        (void)hipEventRecord(ev.b, f->stream);
        st.launches++;
        best.resize(nd); cells.resize(nd);
        HIPCHK(f, hipMemcpyAsync(best.data(), f->x_best.p, nd * 8, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(f, hipMemcpyAsync(cells.data(), f->x_cells.p, nd * 4, hipMemcpyDeviceToHost, f->stream));
        if (trace) {
            k_fm_chain_trace<<<grid_for(nd, 256), 256, 0, f->stream>>>(f->x_jobs.as<FmChainJob>(), f->x_anchors.as<FmChainAnchor>(),
                                                                       (u32)nd, w, f->x_flags.as<u8>(), f->x_best.as<u64>(),
                                                                       nullptr, nullptr, f->x_tr.as<u32>());
            st.launches++;
            tr.resize(4 * nd);
            HIPCHK(f, hipMemcpyAsync(tr.data(), f->x_tr.p, nd * 16, hipMemcpyDeviceToHost, f->stream));
        }
        int rc = fm_sync(f);
        if (rc) return rc;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev.a, ev.b);
        st.ms_kernel += ms;
        for (u64 a = 0; a < nd; a++) st.cells += cells[a];
        u64 total = 0;
        if (trace) {
            coff.resize(nd + 1);
            coff[0] = 0;
            for (u64 a = 0; a < nd; a++) coff[a + 1] = coff[a] + tr[4 * a + 3];
            total = coff[nd];
            ops.resize(total);
            if (total) {
                FM_ENSURE(f, f->x_cig, (size_t)total * 4);
                HIPCHK(f, hipMemcpyAsync(f->x_cigoff.p, coff.data(), (nd + 1) * 8, hipMemcpyHostToDevice, f->stream));
                (void)hipEventRecord(ev.a, f->stream);
                k_fm_chain_trace<<<grid_for(nd, 256), 256, 0, f->stream>>>(f->x_jobs.as<FmChainJob>(),
                                                                           f->x_anchors.as<FmChainAnchor>(), (u32)nd, w,
                                                                           f->x_flags.as<u8>(), f->x_best.as<u64>(),
                                                                           f->x_cigoff.as<u64>(), f->x_cig.as<u32>(),
                                                                           f->x_tr.as<u32>());
                (void)hipEventRecord(ev.b, f->stream);
                st.launches++;
                HIPCHK(f, hipMemcpyAsync(ops.data(), f->x_cig.p, total * 4, hipMemcpyDeviceToHost, f->stream));
                if ((rc = fm_sync(f))) return rc;
                (void)hipEventElapsedTime(&ms, ev.a, ev.b);
                st.ms_trace += ms;
            }
        }
        for (u64 a = 0; a < nd; a++) {
            debwt_fm_aln &o = out[src[a]];
            o = debwt_fm_aln{};
            const u64 key = best[a];
            if (!(key >> 32)) continue;
            const u32 i = 65535u - (u32)((key >> 8) & 0xFFFFu), k = 127u - (u32)(key & 0xFFu);
            const FmChainAnchor *an = da.data() + dj[a].aoff;
            u32 x = dj[a].na - 1;                            // the anchor in effect at the end row
            while (x > 0 && an[x].q > i) x--;
            o.score = (int32_t)(key >> 32);
            o.qend = i + 1;
            o.tend = (u64)(dj[a].tbase + (long long)i + an[x].dc + (long long)k) + 1;
            if (trace) {
                o.qbeg = tr[4 * a]; o.tbeg = (u64)(dj[a].tbase + (long long)(int32_t)tr[4 * a + 1]); o.edits = tr[4 * a + 2];
                (*cig_n)[src[a]] = tr[4 * a + 3];
            }
        }
        if (trace) cig->insert(cig->end(), ops.begin(), ops.end());   // device jobs are in job order
        st.batches++;
        j0 = j1;
    }
    return DEBWT_OK;
}

// |a - b| <= band, for any two diagonals
bool fm_diag_near(int64_t a, int64_t b, u32 band) {
    const __int128 d = (__int128)a - (__int128)b;
    return (d < 0 ? -d : d) <= (__int128)band;
}

}  // namespace

extern "C" int debwt_fm_chain_seeds(const debwt_fm_seed *seeds, uint64_t nseeds, uint32_t band, uint32_t max_gap,
                                    uint32_t max_chains, debwt_fm_chain *chains, debwt_fm_anchor *anchors,
                                    uint64_t anchor_capacity, uint64_t *anchors_needed) {
    if ((nseeds && !seeds) || (max_chains && !chains) || !anchors_needed || band > FM_EXT_MAX_BAND) return DEBWT_EINVAL;
    for (u64 i = 0; i < nseeds; i++)
        if (seeds[i].qend <= seeds[i].qbeg) return DEBWT_EINVAL;
    *anchors_needed = 0;
    typedef __int128 wide;
    struct S { wide tb, te; int64_t diag; u32 strand, record, qb, qe; };
    std::vector<S> s(nseeds);
    u32 longest = 0;
    for (u64 i = 0; i < nseeds; i++) {
        const debwt_fm_seed &x = seeds[i];
        s[i] = S{(wide)x.diag + x.qbeg, (wide)x.diag + x.qend, x.diag, x.strand, x.record, x.qbeg, x.qend};
        longest = std::max(longest, x.qend - x.qbeg);
    }
    std::sort(s.begin(), s.end(), [](const S &a, const S &b) {
        return std::make_tuple(a.strand, a.record, a.tb, a.qb, a.qe) < std::make_tuple(b.strand, b.record, b.tb, b.qb, b.qe);
    });
    std::vector<int64_t> fv(nseeds), pred(nseeds, -1);
    const wide reach = (wide)max_gap + longest;
    for (u64 j = 0; j < nseeds; j++) {
        const S &b = s[j];
        const int64_t len = b.qe - b.qb;
        bool have = false;
        int64_t top = 0, who = -1;
        for (u64 i = j; i-- > 0;) {
            const S &a = s[i];
            if (a.strand != b.strand || a.record != b.record || b.tb - a.tb > reach) break;
            if (!(a.qb < b.qb && a.qe < b.qe && a.tb < b.tb && a.te < b.te) || !fm_diag_near(a.diag, b.diag, band)) continue;
            if ((int64_t)b.qb - (int64_t)a.qe > (int64_t)max_gap || b.tb - a.te > (wide)max_gap) continue;
            const wide dd = (wide)b.diag - (wide)a.diag;
            const int64_t gain = std::min<int64_t>(len, std::min<int64_t>(b.qe - a.qe, (int64_t)(b.te - a.te))) -
                                 (int64_t)(dd < 0 ? -dd : dd);
            const int64_t v = fv[i] + gain;
            if (!have || v > top) { have = true; top = v; who = (int64_t)i; }   // going down: the largest i of a tie stays
        }
        if (have && top >= len) { fv[j] = top; pred[j] = who; } else fv[j] = len;
    }
    std::vector<u64> ord(nseeds);
    for (u64 i = 0; i < nseeds; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](u64 a, u64 b) { return fv[a] > fv[b]; });
    struct C { int64_t score; u64 first, n; };             // first: the chain's seeds in `walk`, end first
    std::vector<C> cs;
    std::vector<u64> walk;
    std::vector<char> used(nseeds, 0);
    for (u64 e : ord) {
        if (used[e]) continue;
        C c{fv[e], walk.size(), 0};
        int64_t p = (int64_t)e;
        for (; p >= 0 && !used[p]; p = pred[p]) { walk.push_back((u64)p); c.n++; }
        if (p >= 0) c.score -= fv[p];
        for (u64 x = c.first; x < c.first + c.n; x++) used[walk[x]] = 1;
        cs.push_back(c);
    }
    auto head = [&](const C &c) -> const S & { return s[walk[c.first + c.n - 1]]; };
    std::stable_sort(cs.begin(), cs.end(), [&](const C &a, const C &b) {
        if (a.score != b.score) return a.score > b.score;
        const S &x = head(a), &y = head(b);
        return std::make_tuple(x.strand, x.record, x.diag, x.qb) < std::make_tuple(y.strand, y.record, y.diag, y.qb);
    });
    const u64 k = std::min<u64>(cs.size(), max_chains);
    u64 need = 0;
    for (u64 c = 0; c < k; c++) {
        chains[c] = debwt_fm_chain{(int32_t)cs[c].score, head(cs[c]).record, head(cs[c]).strand, (u32)cs[c].n, need};
        need += cs[c].n;
    }
    *anchors_needed = need;
    if (anchor_capacity < need || (need && !anchors)) return DEBWT_ERANGE;
    for (u64 c = 0; c < k; c++)
        for (u64 x = 0; x < cs[c].n; x++) {
            const S &y = s[walk[cs[c].first + cs[c].n - 1 - x]];
            anchors[chains[c].first_anchor + x] = debwt_fm_anchor{y.qb, 0, y.diag};
        }
    return (int)k;
}

extern "C" int debwt_fm_extend_chain(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                                     const debwt_fm_chain_job *jobs, uint64_t njobs, const debwt_fm_anchor *anchors,
                                     uint64_t nanchors, const debwt_fm_scoring *sc, uint32_t band, debwt_fm_aln *out,
                                     uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity) {
    if (!f || !sc || !offsets || (njobs && (!jobs || !out)) || (nanchors && !anchors)) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->x_stats = debwt_fm_extend_stats{};
    int rc = fm_ext_check(f, sc, band, "debwt_fm_extend_chain");
    if (rc) return rc;
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_extend_chain: offsets must not decrease"; return DEBWT_EINVAL; }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    for (u64 j = 0; j < njobs; j++) {
        const debwt_fm_chain_job &jb = jobs[j];
        const std::string who = "debwt_fm_extend_chain: job " + std::to_string(j);
        if (jb.pattern >= npat || jb.strand > 1 || jb.record >= f->nrec) {
            f->err = who + " names a pattern, strand or record that does not exist";
            return DEBWT_EINVAL;
        }
        const u64 m = offsets[jb.pattern + 1] - offsets[jb.pattern];
        if (m < 1 || m > FM_EXT_MAX_LEN) {
            f->err = who + " has a pattern of " + std::to_string(m) + " bytes (1..65535)";
            return DEBWT_EINVAL;
        }
        if (!jb.n_anchors || jb.first_anchor > nanchors || jb.n_anchors > nanchors - jb.first_anchor) {
            f->err = who + " has no anchor, or anchors outside the " + std::to_string(nanchors) + " given";
            return DEBWT_EINVAL;
        }
        const debwt_fm_anchor *an = anchors + jb.first_anchor;
        for (u32 a = 0; a < jb.n_anchors; a++) {
            if (an[a].qbeg >= m || (a && an[a].qbeg <= an[a - 1].qbeg)) {
                f->err = who + ": the qbeg of its anchors must increase strictly and stay below the pattern length";
                return DEBWT_EINVAL;
            }
            if (a && !fm_diag_near(an[a].diag, an[a - 1].diag, band)) {
                f->err = who + ": consecutive anchors lie further apart than the band";
                return DEBWT_EINVAL;
            }
        }
    }
    HIPCHK(f, hipSetDevice(f->device));
    const bool trace = cigar_offsets != nullptr;
    std::vector<u32> cig_n, cig;
    rc = fm_chain_run(f, patterns, offsets, jobs, njobs, anchors, *sc, band, trace, out, &cig_n, &cig);
    if (rc) return rc;
    f->x_stats.ms_wall = (float)fm_ms_since(t0);
    if (!trace) return DEBWT_OK;
    cigar_offsets[0] = 0;
    for (u64 j = 0; j < njobs; j++) cigar_offsets[j + 1] = cigar_offsets[j] + cig_n[j];
    if (capacity < cig.size() || (!cig.empty() && !cigar)) {
        f->err = "debwt_fm_extend_chain: capacity below the CIGAR ops (cigar_offsets[njobs] = " + std::to_string(cig.size()) + ")";
        return DEBWT_ERANGE;
    }
    if (!cig.empty()) memcpy(cigar, cig.data(), cig.size() * 4);
    return DEBWT_OK;
}

extern "C" void debwt_fm_chain_defaults(debwt_fm_chain_opts *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    debwt_fm_map_defaults(&o->map);
    o->max_gap = 5000;
}

extern "C" int debwt_fm_map_chained(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                                    const debwt_fm_chain_opts *opts, debwt_fm_hit *hits, uint64_t *cigar_offsets,
                                    uint32_t *cigar, uint64_t capacity, uint64_t *anchor_offsets,
                                    debwt_fm_anchor *hit_anchors, uint64_t anchor_capacity) {
    if (!f || !offsets || !cigar_offsets || (npat && !hits)) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    debwt_fm_chain_opts co;
    debwt_fm_chain_defaults(&co);
    if (opts) co = *opts;
    const debwt_fm_map_opts &o = co.map;
    f->map_stats = debwt_fm_map_stats{};
    f->x_stats = debwt_fm_extend_stats{};
    int rc = fm_ext_check(f, &o.scoring, o.band, "debwt_fm_map_chained");
    if (rc) return rc;
    if (!o.min_len || !o.max_occ || !o.max_cand || o.max_cand > 4096 || (o.flags & ~DEBWT_FM_MAP_FORWARD)) {
        f->err = "debwt_fm_map_chained: min_len, max_occ and max_cand must be positive (max_cand <= 4096), flags known";
        return DEBWT_EINVAL;
    }
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_map_chained: offsets must not decrease"; return DEBWT_EINVAL; }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    debwt_fm_map_stats &ms = f->map_stats;
    ms.reads = npat;
    cigar_offsets[0] = 0;
    if (anchor_offsets) anchor_offsets[0] = 0;
    std::vector<u32> all_cig;
    std::vector<debwt_fm_anchor> all_anchors;
    std::vector<uint64_t> moff, ranges, loff, pos;
    std::vector<u32> spans, cig_n, cig;
    std::vector<u8> strands;
    std::vector<debwt_fm_chain_job> jobs;
    std::vector<debwt_fm_anchor> anchors;
    std::vector<u64> job_first;
    std::vector<debwt_fm_aln> aln;
    const u32 mflags = (o.flags & DEBWT_FM_MAP_FORWARD) ? 0u : DEBWT_FM_BOTH_STRANDS;
    for (u64 p0 = 0; p0 < npat;) {
        u64 p1 = p0 + 1;
        while (p1 < npat && p1 - p0 < (1ull << 18) && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS) p1++;
        const u64 np = p1 - p0;
        // 1. MEMs of the batch
        auto t = std::chrono::steady_clock::now();
        moff.assign(np + 1, 0);
        u64 cap = std::max<u64>(spans.size() / 2, 4 * np + 16);
        for (;;) {
            spans.resize(2 * cap); ranges.resize(2 * cap); strands.resize(cap);
            rc = debwt_fm_mems(f, patterns, offsets + p0, np, o.min_len, mflags, moff.data(), spans.data(), ranges.data(),
                               strands.data(), cap);
            if (rc == DEBWT_ERANGE && moff[np] > cap) { cap = moff[np]; continue; }
            if (rc) return rc;
            break;
        }
        const u64 nmem = moff[np];
        ms.mems += nmem;
        ms.ms_mems += (float)fm_ms_since(t);
        // 2. their first max_occ rows located
        t = std::chrono::steady_clock::now();
        loff.assign(nmem + 1, 0);
        u64 nocc = 0;
        for (u64 i = 0; i < nmem; i++) nocc += std::min<u64>(ranges[2 * i + 1] - ranges[2 * i], o.max_occ);
        pos.resize(std::max<u64>(nocc, 1));
        rc = debwt_fm_locate(f, ranges.data(), nmem, o.max_occ, loff.data(), pos.data(), pos.size());
        if (rc) return rc;
        ms.seeds += nocc;
        ms.ms_locate += (float)fm_ms_since(t);
        // 3. seeds -> chains -> jobs: every read on its own, the reads spread over at most 16 threads
        t = std::chrono::steady_clock::now();
        struct PerRead { std::vector<debwt_fm_chain> chains; std::vector<debwt_fm_anchor> anchors; };
        std::vector<PerRead> per(np);
        std::atomic<u64> next{0};
        std::atomic<int> bad{0};
        auto worker = [&]() {
            std::vector<debwt_fm_seed> seeds;
            for (;;) {
                const u64 r0 = next.fetch_add(64);
                if (r0 >= np) return;
                for (u64 r = r0; r < std::min(np, r0 + 64); r++) {
                    const u64 m = offsets[p0 + r + 1] - offsets[p0 + r];
                    if (m < 1 || m > FM_EXT_MAX_LEN) continue;
                    seeds.clear();
                    for (u64 i = moff[r]; i < moff[r + 1]; i++) {
                        const u32 qb = strands[i] ? (u32)m - spans[2 * i + 1] : spans[2 * i];      // in Q
                        const u32 qe = strands[i] ? (u32)m - spans[2 * i] : spans[2 * i + 1];
                        for (u64 x = loff[i]; x < loff[i + 1]; x++) {
                            const u64 tp = pos[x];
                            const u64 rec = (u64)(std::upper_bound(f->rec_starts.begin(), f->rec_starts.end(), tp) - f->rec_starts.begin()) - 1;
                            seeds.push_back(debwt_fm_seed{(int64_t)tp - (int64_t)qb, (u32)rec, strands[i], qb, qe});
                        }
                    }
                    if (seeds.empty()) continue;
                    PerRead &pr = per[r];
                    pr.chains.resize(o.max_cand);
                    pr.anchors.resize(seeds.size());                       // chains share no seed
                    uint64_t need = 0;
                    const int nc = debwt_fm_chain_seeds(seeds.data(), seeds.size(), o.band, co.max_gap, o.max_cand,
                                                        pr.chains.data(), pr.anchors.data(), pr.anchors.size(), &need);
                    if (nc < 0) { bad.store(1); pr.chains.clear(); continue; }
                    pr.chains.resize((size_t)nc);
                    pr.anchors.resize(need);
                }
            }
        };
        {
            const unsigned nt = (unsigned)std::max<u64>(1, std::min<u64>({16, (u64)std::thread::hardware_concurrency(), (np + 63) / 64}));
            std::vector<std::thread> th;
            for (unsigned x = 1; x < nt; x++) th.emplace_back(worker);
            worker();
            for (auto &x : th) x.join();
        }
        if (bad.load()) { f->err = "debwt_fm_map_chained: a MEM with an empty span"; return DEBWT_EINTERNAL; }
        jobs.clear(); anchors.clear();
        job_first.assign(np + 1, 0);
        for (u64 r = 0; r < np; r++) {
            job_first[r] = jobs.size();
            for (const debwt_fm_chain &c : per[r].chains) {
                jobs.push_back(debwt_fm_chain_job{p0 + r, c.record, c.strand, anchors.size() + c.first_anchor, c.n_anchors, 0});
            }
            anchors.insert(anchors.end(), per[r].anchors.begin(), per[r].anchors.end());
        }
        job_first[np] = jobs.size();
        ms.candidates += jobs.size();
        ms.jobs += jobs.size();
        ms.ms_candidates += (float)fm_ms_since(t);
        // 4. every chain extended, with its traceback: the tie rule and `sub` need the text interval of each
        t = std::chrono::steady_clock::now();
        aln.resize(jobs.size());
        HIPCHK(f, hipSetDevice(f->device));
        rc = fm_chain_run(f, patterns, offsets, jobs.data(), jobs.size(), anchors.data(), o.scoring, o.band, true, aln.data(),
                          &cig_n, &cig);
        if (rc) return rc;
        ms.ms_extend += (float)fm_ms_since(t);
        // 5. the winner of every read
        std::vector<u64> cfirst(jobs.size() + 1, 0);
        for (u64 j = 0; j < jobs.size(); j++) cfirst[j + 1] = cfirst[j] + cig_n[j];
        for (u64 r = 0; r < np; r++) {
            const u64 m = offsets[p0 + r + 1] - offsets[p0 + r];
            debwt_fm_hit &h = hits[p0 + r];
            memset(&h, 0, sizeof h);
            h.pattern = p0 + r;
            h.flags = DEBWT_FM_MAP_UNMAPPED | (m > FM_EXT_MAX_LEN ? DEBWT_FM_MAP_TOO_LONG : 0u);
            cigar_offsets[p0 + r + 1] = cigar_offsets[p0 + r];
            if (anchor_offsets) anchor_offsets[p0 + r + 1] = anchor_offsets[p0 + r];
            u64 w = ~0ull;
            for (u64 j = job_first[r]; j < job_first[r + 1]; j++) {
                if (aln[j].score <= 0) continue;
                if (w == ~0ull || aln[j].score > aln[w].score ||
                    (aln[j].score == aln[w].score && std::make_tuple(jobs[j].strand, jobs[j].record, aln[j].tbeg) <
                                                         std::make_tuple(jobs[w].strand, jobs[w].record, aln[w].tbeg)))
                    w = j;
            }
            if (w == ~0ull || aln[w].score < o.min_score) continue;
            int32_t sub = 0;
            for (u64 j = job_first[r]; j < job_first[r + 1]; j++)
                if (j != w && aln[j].score > sub && (aln[j].tend <= aln[w].tbeg || aln[j].tbeg >= aln[w].tend)) sub = aln[j].score;
            const debwt_fm_aln &a = aln[w];
            h.flags = jobs[w].strand ? DEBWT_FM_MAP_REVERSE : 0u;
            h.record = jobs[w].record; h.offset = a.tbeg - f->rec_starts[jobs[w].record];
            h.qbeg = a.qbeg; h.qend = a.qend; h.tbeg = a.tbeg; h.tend = a.tend;
            h.score = a.score; h.sub = sub; h.mapq = (u32)(60 * (int64_t)(a.score - sub) / a.score); h.edits = a.edits;
            h.diag = anchors[jobs[w].first_anchor].diag;
            all_cig.insert(all_cig.end(), cig.begin() + cfirst[w], cig.begin() + cfirst[w + 1]);
            cigar_offsets[p0 + r + 1] = all_cig.size();
            if (anchor_offsets) {
                all_anchors.insert(all_anchors.end(), anchors.begin() + jobs[w].first_anchor,
                                   anchors.begin() + jobs[w].first_anchor + jobs[w].n_anchors);
                anchor_offsets[p0 + r + 1] = all_anchors.size();
            }
            ms.mapped++;
        }
        ms.batches++;
        p0 = p1;
    }
    f->x_stats.ms_wall = ms.ms_extend;
    ms.ms_wall = (float)fm_ms_since(t0);
    rc = DEBWT_OK;
    if (capacity < all_cig.size() || (!all_cig.empty() && !cigar)) {
        f->err = "debwt_fm_map_chained: capacity below the CIGAR ops (cigar_offsets[npat] = " + std::to_string(all_cig.size()) + ")";
        rc = DEBWT_ERANGE;
    }
    if (anchor_offsets && (anchor_capacity < all_anchors.size() || (!all_anchors.empty() && !hit_anchors))) {
        f->err = "debwt_fm_map_chained: anchor capacity below the anchors (anchor_offsets[npat] = " + std::to_string(all_anchors.size()) + ")";
        rc = DEBWT_ERANGE;
    }
    if (rc) return rc;
    if (!all_cig.empty()) memcpy(cigar, all_cig.data(), all_cig.size() * 4);
    if (anchor_offsets && !all_anchors.empty()) memcpy(hit_anchors, all_anchors.data(), all_anchors.size() * sizeof(debwt_fm_anchor));
    return DEBWT_OK;
}

// ---- paired ends: alignment against a text window, insert bounds, pair selection, the pair mapper (fm_window_kernels.h) --
// The batches, the two traceback passes and the statistics are those of fm_extend_run; a job's flag scratch is 64 bytes
// per step of its wave, a wave step being one anti-diagonal of one strip of 64 window columns.

namespace {

// the device form of a window job; false: the window misses the record (score 0)
bool fm_win_prepare(const debwt_fm *f, u64 m, const debwt_fm_window_job &jb, FmWinJob *d) {
    const u64 rs = f->rec_starts[jb.record];
    const u64 re = (jb.record + 1 < f->nrec ? f->rec_starts[jb.record + 1] : f->n) - 1;
    const u64 lo = std::max<u64>(rs, jb.wbeg), hi = std::min<u64>(re, jb.wend);
    if (lo >= hi) return false;
    d->qoff = 0; d->flag_off = 0; d->tbase = lo;
    d->m = (u32)m; d->strand = jb.strand;
    d->ncol = (u32)(hi - lo); d->nstrips = (d->ncol + 63) / 64;
    return true;
}

u64 fm_win_steps(const FmWinJob &d) {                     // steps of the job's wave over all strips
    return (u64)(d.nstrips - 1) * (d.m + 63) + d.m + (d.ncol - 64 * (d.nstrips - 1)) - 1;
}

// jobs [0, njobs) -> out; with `trace` also ops per job (cig_n) and the ops of all jobs in job order (cig).  The
// arguments were validated by the caller; statistics are added to f->x_stats.
int fm_window_run(debwt_fm *f, const char *patterns, const uint64_t *offsets, const debwt_fm_window_job *jobs, u64 njobs,
                  const debwt_fm_scoring &sc, bool trace, debwt_fm_aln *out, std::vector<u32> *cig_n, std::vector<u32> *cig) {
    debwt_fm_extend_stats &st = f->x_stats;
    st.jobs += njobs;
    if (trace) { cig_n->assign(njobs, 0); cig->clear(); }
    if (!njobs) return DEBWT_OK;
    const u64 limit = fm_env_u64("DEBWT_FM_EXTEND_BYTES", FM_EXTEND_BYTES);
    FmEvents ev;
    if (int rc = ev.init(f)) return rc;
    std::vector<FmWinJob> dj;
    std::vector<u64> src;                                // job index of every device job
    std::vector<char> chars;
    std::vector<u64> best;
    std::vector<u32> cells, tr, ops;
    std::vector<u64> coff;
    for (u64 j0 = 0; j0 < njobs;) {
        dj.clear(); src.clear(); chars.clear();
        u64 fbytes = 0, j1 = j0, last_pat = ~0ull, last_off = 0, steps = 0;
        u32 lds_job = 8;
        for (; j1 < njobs; j1++) {
            const debwt_fm_window_job &jb = jobs[j1];
            const u64 m = offsets[jb.pattern + 1] - offsets[jb.pattern];
            FmWinJob d;
            if (!fm_win_prepare(f, m, jb, &d)) { out[j1] = debwt_fm_aln{}; continue; }
            const u64 ns = fm_win_steps(d), fb = trace ? 64 * ns : 0;
            const bool fresh = jb.pattern != last_pat;
            if (!dj.empty() && (fbytes + fb > limit || dj.size() >= FM_EXTEND_JOBS ||
                                (fresh && chars.size() + m > FM_BATCH_CHARS)))
                break;
            if (fresh) {
                last_pat = jb.pattern; last_off = chars.size();
                chars.insert(chars.end(), patterns + offsets[jb.pattern], patterns + offsets[jb.pattern] + m);
            }
            d.qoff = last_off; d.flag_off = fbytes;
            fbytes += fb; steps += ns;
            lds_job = std::max(lds_job, fm_win_lds(d.m, d.ncol));
            dj.push_back(d); src.push_back(j1);
        }
        const u64 nd = dj.size();
        if (!nd) { j0 = j1; continue; }
        // the workgroup: as many waves (1..4), one job each, as the staged strings and hand-over buffers leave room for
        const u32 jpb = std::max<u32>(1, std::min<u32>(4, FM_EXT_LDS_BUDGET / lds_job));
        const u32 block = 64 * jpb, grid = (u32)((nd + jpb - 1) / jpb);
        st.wave_steps += steps;
        st.scratch_bytes = std::max<u64>(st.scratch_bytes, fbytes);
        FM_ENSURE(f, f->q_chars, std::max<size_t>(chars.size(), 1));
        FM_ENSURE(f, f->x_jobs, nd * sizeof(FmWinJob));
        FM_ENSURE(f, f->x_best, nd * 8);
        FM_ENSURE(f, f->x_cells, nd * 4);
        if (trace) {
            FM_ENSURE(f, f->x_flags, (size_t)std::max<u64>(fbytes, 1));
            FM_ENSURE(f, f->x_tr, nd * 16);
            FM_ENSURE(f, f->x_cigoff, (nd + 1) * 8);
        }
        HIPCHK(f, hipMemcpyAsync(f->q_chars.p, chars.data(), chars.size(), hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(f->x_jobs.p, dj.data(), nd * sizeof(FmWinJob), hipMemcpyHostToDevice, f->stream));
        (void)hipEventRecord(ev.a, f->stream);
        const size_t lds = (size_t)jpb * lds_job;
        if (trace)
            k_fm_window<true><<<grid, block, lds, f->stream>>>(f->text.as<u64>(), f->q_chars.as<u8>(), f->x_jobs.as<FmWinJob>(),
                                                               (u32)nd, sc.match, sc.mismatch, sc.gap_open, sc.gap_extend,
                                                               lds_job, f->x_flags.as<u8>(), f->x_best.as<u64>(),
                                                               f->x_cells.as<u32>());
        else
            k_fm_window<false><<<grid, block, lds, f->stream>>>(f->text.as<u64>(), f->q_chars.as<u8>(), f->x_jobs.as<FmWinJob>(),
                                                                (u32)nd, sc.match, sc.mismatch, sc.gap_open, sc.gap_extend,
                                                                lds_job, f->x_flags.as<u8>(), f->x_best.as<u64>(),
                                                                f->x_cells.as<u32>());
        (void)hipEventRecord(ev.b, f->stream);
        st.launches++;
        best.resize(nd); cells.resize(nd);
        HIPCHK(f, hipMemcpyAsync(best.data(), f->x_best.p, nd * 8, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(f, hipMemcpyAsync(cells.data(), f->x_cells.p, nd * 4, hipMemcpyDeviceToHost, f->stream));
        if (trace) {
            k_fm_window_trace<<<grid_for(nd, 256), 256, 0, f->stream>>>(f->x_jobs.as<FmWinJob>(), (u32)nd, f->x_flags.as<u8>(),
                                                                        f->x_best.as<u64>(), nullptr, nullptr, f->x_tr.as<u32>());
            st.launches++;
            tr.resize(4 * nd);
            HIPCHK(f, hipMemcpyAsync(tr.data(), f->x_tr.p, nd * 16, hipMemcpyDeviceToHost, f->stream));
        }
        int rc = fm_sync(f);
        if (rc) return rc;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev.a, ev.b);
        st.ms_kernel += ms;
        for (u64 a = 0; a < nd; a++) st.cells += cells[a];
        u64 total = 0;
        if (trace) {
            coff.resize(nd + 1);
            coff[0] = 0;
            for (u64 a = 0; a < nd; a++) coff[a + 1] = coff[a] + tr[4 * a + 3];
            total = coff[nd];
            ops.resize(total);
            if (total) {
                FM_ENSURE(f, f->x_cig, (size_t)total * 4);
                HIPCHK(f, hipMemcpyAsync(f->x_cigoff.p, coff.data(), (nd + 1) * 8, hipMemcpyHostToDevice, f->stream));
                (void)hipEventRecord(ev.a, f->stream);
                k_fm_window_trace<<<grid_for(nd, 256), 256, 0, f->stream>>>(f->x_jobs.as<FmWinJob>(), (u32)nd, f->x_flags.as<u8>(),
                                                                            f->x_best.as<u64>(), f->x_cigoff.as<u64>(),
                                                                            f->x_cig.as<u32>(), f->x_tr.as<u32>());
                (void)hipEventRecord(ev.b, f->stream);
                st.launches++;
                HIPCHK(f, hipMemcpyAsync(ops.data(), f->x_cig.p, total * 4, hipMemcpyDeviceToHost, f->stream));
                if ((rc = fm_sync(f))) return rc;
                (void)hipEventElapsedTime(&ms, ev.a, ev.b);
                st.ms_trace += ms;
            }
        }
        for (u64 a = 0; a < nd; a++) {
            debwt_fm_aln &o = out[src[a]];
            o = debwt_fm_aln{};
            const u64 key = best[a];
            if (!(key >> 32)) continue;
            const u32 i = 4095u - (u32)((key >> 14) & 0xFFFu), c = 16383u - (u32)(key & 0x3FFFu);
            o.score = (int32_t)(key >> 32);
            o.qend = i + 1;
            o.tend = dj[a].tbase + c + 1;
            if (trace) {
                o.qbeg = tr[4 * a]; o.tbeg = dj[a].tbase + tr[4 * a + 1]; o.edits = tr[4 * a + 2];
                (*cig_n)[src[a]] = tr[4 * a + 3];
            }
        }
        if (trace) cig->insert(cig->end(), ops.begin(), ops.end());   // device jobs are in job order
        st.batches++;
        j0 = j1;
    }
    return DEBWT_OK;
}

// the checks of debwt_fm_align_window, then the run; x_stats are those of this pass
int fm_window_call(debwt_fm *f, const char *patterns, const uint64_t *offsets, u64 npat, const debwt_fm_window_job *jobs,
                   u64 njobs, const debwt_fm_scoring *sc, bool trace, debwt_fm_aln *out, std::vector<u32> *cig_n,
                   std::vector<u32> *cig) {
    const auto t0 = std::chrono::steady_clock::now();
    f->x_stats = debwt_fm_extend_stats{};
    int rc = fm_ext_check(f, sc, 0, "debwt_fm_align_window");
    if (rc) return rc;
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_align_window: offsets must not decrease"; return DEBWT_EINVAL; }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    for (u64 j = 0; j < njobs; j++) {
        const debwt_fm_window_job &jb = jobs[j];
        const std::string who = "debwt_fm_align_window: job " + std::to_string(j);
        if (jb.pattern >= npat || jb.strand > 1 || jb.record >= f->nrec) {
            f->err = who + " names a pattern, strand or record that does not exist";
            return DEBWT_EINVAL;
        }
        const u64 m = offsets[jb.pattern + 1] - offsets[jb.pattern];
        if (m < 1 || m > DEBWT_FM_WINDOW_MAX_QUERY) {
            f->err = who + " has a pattern of " + std::to_string(m) + " bytes (1..4096)";
            return DEBWT_EINVAL;
        }
        if (jb.wend < jb.wbeg || jb.wend - jb.wbeg > DEBWT_FM_WINDOW_MAX_COLUMNS) {
            f->err = who + " has a window that ends before it begins or is wider than 16384";
            return DEBWT_EINVAL;
        }
    }
    HIPCHK(f, hipSetDevice(f->device));
    rc = fm_window_run(f, patterns, offsets, jobs, njobs, *sc, trace, out, cig_n, cig);
    if (rc) return rc;
    f->x_stats.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

}  // namespace

static_assert(DEBWT_FM_WINDOW_MAX_QUERY == FM_WIN_MAX_LEN && DEBWT_FM_WINDOW_MAX_COLUMNS == FM_WIN_MAX_COLS,
              "the limits of the header are those of the kernel's key");

extern "C" int debwt_fm_align_window(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                                     const debwt_fm_window_job *jobs, uint64_t njobs, const debwt_fm_scoring *sc,
                                     debwt_fm_aln *out, uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity) {
    if (!f || !sc || !offsets || (njobs && (!jobs || !out))) return DEBWT_EINVAL;
    const bool trace = cigar_offsets != nullptr;
    std::vector<u32> cig_n, cig;
    const int rc = fm_window_call(f, patterns, offsets, npat, jobs, njobs, sc, trace, out, &cig_n, &cig);
    if (rc) return rc;
    if (!trace) return DEBWT_OK;
    cigar_offsets[0] = 0;
    for (u64 j = 0; j < njobs; j++) cigar_offsets[j + 1] = cigar_offsets[j] + cig_n[j];
    if (capacity < cig.size() || (!cig.empty() && !cigar)) {
        f->err = "debwt_fm_align_window: capacity below the CIGAR ops (cigar_offsets[njobs] = " + std::to_string(cig.size()) + ")";
        return DEBWT_ERANGE;
    }
    if (!cig.empty()) memcpy(cigar, cig.data(), cig.size() * 4);
    return DEBWT_OK;
}

extern "C" int debwt_fm_insert_bounds(const uint64_t *tlen, uint64_t n, uint32_t *lo, uint32_t *hi) {
    if (!tlen || !lo || !hi || n < DEBWT_FM_INSERT_MIN_PAIRS) return DEBWT_EINVAL;
    std::vector<u64> s(tlen, tlen + n);
    std::sort(s.begin(), s.end());
    const __int128 q1 = s[n / 4], q3 = s[3 * n / 4], d = q3 - q1;
    const __int128 l = std::max<__int128>(1, q1 - 3 * d), h = std::min<__int128>(DEBWT_FM_INSERT_MAX, q3 + 3 * d);
    *lo = (uint32_t)std::min<__int128>(l, 0xFFFFFFFFu);
    *hi = (uint32_t)h;
    return DEBWT_OK;
}

namespace {

bool fm_pair_disjoint(const debwt_fm_pcand &a, const debwt_fm_pcand &b) { return a.tend <= b.tbeg || a.tbeg >= b.tend; }

// a proper pair by the header's rule; T and the forward mate's tbeg for the caller
bool fm_pair_proper(const debwt_fm_pcand &a, const debwt_fm_pcand &b, int32_t thr, u32 lo, u32 hi, u64 *T, u64 *tbf) {
    if (a.score < thr || b.score < thr || a.record != b.record || a.strand > 1 || b.strand > 1 || a.strand == b.strand)
        return false;
    const debwt_fm_pcand &fw = a.strand ? b : a, &rv = a.strand ? a : b;
    if (fw.tbeg > rv.tbeg || fw.tend > rv.tend) return false;
    *T = rv.tend - fw.tbeg; *tbf = fw.tbeg;
    return *T >= lo && *T <= hi;
}

// b(x): the eligible candidate of largest score, ties by smaller (strand, record, tbeg), then by smaller index
int32_t fm_pair_single(const debwt_fm_pcand *c, u32 n, int32_t thr) {
    int32_t b = -1;
    for (u32 i = 0; i < n; i++) {
        if (c[i].score < thr) continue;
        if (b < 0 || c[i].score > c[b].score ||
            (c[i].score == c[b].score && std::make_tuple(c[i].strand, c[i].record, c[i].tbeg) <
                                             std::make_tuple(c[b].strand, c[b].record, c[b].tbeg)))
            b = (int32_t)i;
    }
    return b;
}

int32_t fm_pair_sub(const debwt_fm_pcand *c, u32 n, int32_t w) {
    int32_t sub = 0;
    if (w < 0) return 0;
    for (u32 k = 0; k < n; k++)
        if ((int32_t)k != w && c[k].score > sub && fm_pair_disjoint(c[k], c[w])) sub = c[k].score;
    return sub;
}

}  // namespace

extern "C" int debwt_fm_pair_select(const debwt_fm_pcand *c1, uint32_t n1, const debwt_fm_pcand *c2, uint32_t n2,
                                    uint32_t ins_lo, uint32_t ins_hi, int32_t unpaired_penalty, int32_t min_score,
                                    debwt_fm_pair_choice *out) {
    if (!out || (n1 && !c1) || (n2 && !c2) || ins_lo > ins_hi || n1 > 0x7FFFFFFFu || n2 > 0x7FFFFFFFu) return DEBWT_EINVAL;
    for (u32 i = 0; i < n1; i++) if (c1[i].score > 0 && c1[i].tend <= c1[i].tbeg) return DEBWT_EINVAL;
    for (u32 j = 0; j < n2; j++) if (c2[j].score > 0 && c2[j].tend <= c2[j].tbeg) return DEBWT_EINVAL;
    const int32_t thr = std::max<int32_t>(1, min_score);
    const int32_t b1 = fm_pair_single(c1, n1, thr), b2 = fm_pair_single(c2, n2, thr);
    int32_t pi = -1, pj = -1;
    int64_t P = 0;
    u64 pT = 0, ptb = 0;
    for (u32 i = 0; i < n1; i++)
        for (u32 j = 0; j < n2; j++) {
            u64 T, tb;
            if (!fm_pair_proper(c1[i], c2[j], thr, ins_lo, ins_hi, &T, &tb)) continue;
            const int64_t p = (int64_t)c1[i].score + c2[j].score;
            if (pi < 0 || p > P || (p == P && std::make_tuple(c1[i].record, tb) < std::make_tuple(c1[pi].record, ptb))) {
                pi = (int32_t)i; pj = (int32_t)j; P = p; pT = T; ptb = tb;
            }
        }
    debwt_fm_pair_choice ch{};
    const bool proper = pi >= 0 && P >= (int64_t)c1[b1].score + c2[b2].score - unpaired_penalty;
    ch.i1 = proper ? pi : b1; ch.i2 = proper ? pj : b2;
    ch.proper = proper ? 1u : 0u;
    ch.sub1 = fm_pair_sub(c1, n1, ch.i1); ch.sub2 = fm_pair_sub(c2, n2, ch.i2);
    int64_t q1 = 0, q2 = 0;
    if (ch.i1 >= 0) q1 = 60 * (int64_t)(c1[ch.i1].score - ch.sub1) / c1[ch.i1].score;
    if (ch.i2 >= 0) q2 = 60 * (int64_t)(c2[ch.i2].score - ch.sub2) / c2[ch.i2].score;
    if (proper) {
        int64_t psub = 0;
        for (u32 i = 0; i < n1; i++)
            for (u32 j = 0; j < n2; j++) {
                u64 T, tb;
                if (!fm_pair_proper(c1[i], c2[j], thr, ins_lo, ins_hi, &T, &tb)) continue;
                if (!fm_pair_disjoint(c1[i], c1[pi]) && !fm_pair_disjoint(c2[j], c2[pj])) continue;
                psub = std::max<int64_t>(psub, (int64_t)c1[i].score + c2[j].score);
            }
        ch.tlen = (int64_t)pT; ch.pair_score = (int32_t)P; ch.pair_sub = (int32_t)psub;
        const int64_t qp = 60 * (P - psub) / P;
        q1 = std::max(q1, qp); q2 = std::max(q2, qp);
    }
    ch.mapq1 = (u32)std::max<int64_t>(q1, 0); ch.mapq2 = (u32)std::max<int64_t>(q2, 0);
    *out = ch;
    return DEBWT_OK;
}

namespace {

struct FmPairCand {
    debwt_fm_aln a;
    int64_t diag;
    u32 record, strand, rescued, cig_n;
    u64 cig_first;           // in the pool of CIGAR ops
};

// The stages of debwt_fm_map that the pair mapper shares with it -- MEMs, locate, cluster, extend -- over all reads, from
// the same public pieces; every job's alignment is kept: those of read r are cands[first[r] .. first[r + 1]).
int fm_pair_candidates(debwt_fm *f, const char *patterns, const uint64_t *offsets, u64 npat, const debwt_fm_map_opts &o,
                       std::vector<FmPairCand> &cands, std::vector<u64> &first, std::vector<u32> &pool) {
    std::vector<uint64_t> moff, ranges, loff, pos;
    std::vector<u32> spans, cig_n, cig;
    std::vector<u8> strands;
    std::vector<debwt_fm_seed> seeds;
    std::vector<debwt_fm_cand> cand(o.max_cand);
    std::vector<debwt_fm_job> jobs;
    std::vector<debwt_fm_aln> aln;
    cands.clear(); pool.clear();
    first.assign(npat + 1, 0);
    int rc;
    for (u64 p0 = 0; p0 < npat;) {
        u64 p1 = p0 + 1;
        while (p1 < npat && p1 - p0 < (1ull << 18) && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS) p1++;
        const u64 np = p1 - p0;
        moff.assign(np + 1, 0);
        u64 cap = std::max<u64>(spans.size() / 2, 4 * np + 16);
        for (;;) {
            spans.resize(2 * cap); ranges.resize(2 * cap); strands.resize(cap);
            rc = debwt_fm_mems(f, patterns, offsets + p0, np, o.min_len, DEBWT_FM_BOTH_STRANDS, moff.data(), spans.data(),
                               ranges.data(), strands.data(), cap);
            if (rc == DEBWT_ERANGE && moff[np] > cap) { cap = moff[np]; continue; }
            if (rc) return rc;
            break;
        }
        const u64 nmem = moff[np];
        loff.assign(nmem + 1, 0);
        u64 nocc = 0;
        for (u64 i = 0; i < nmem; i++) nocc += std::min<u64>(ranges[2 * i + 1] - ranges[2 * i], o.max_occ);
        pos.resize(std::max<u64>(nocc, 1));
        rc = debwt_fm_locate(f, ranges.data(), nmem, o.max_occ, loff.data(), pos.data(), pos.size());
        if (rc) return rc;
        jobs.clear();
        std::vector<u64> job_first(np + 1, 0);
        for (u64 r = 0; r < np; r++) {
            job_first[r] = jobs.size();
            const u64 m = offsets[p0 + r + 1] - offsets[p0 + r];
            if (m < 1 || m > FM_EXT_MAX_LEN) continue;
            seeds.clear();
            for (u64 i = moff[r]; i < moff[r + 1]; i++) {
                const u32 qb = strands[i] ? (u32)m - spans[2 * i + 1] : spans[2 * i];      // in Q
                const u32 qe = strands[i] ? (u32)m - spans[2 * i] : spans[2 * i + 1];
                for (u64 x = loff[i]; x < loff[i + 1]; x++) {
                    const u64 tp = pos[x];
                    const u64 rec = (u64)(std::upper_bound(f->rec_starts.begin(), f->rec_starts.end(), tp) - f->rec_starts.begin()) - 1;
                    seeds.push_back(debwt_fm_seed{(int64_t)tp - (int64_t)qb, (u32)rec, strands[i], qb, qe});
                }
            }
            if (seeds.empty()) continue;
            const int nc = debwt_fm_cluster_seeds(seeds.data(), seeds.size(), o.band, o.max_cand, cand.data());
            if (nc < 0) { f->err = "debwt_fm_map_pairs: a MEM with an empty span"; return DEBWT_EINTERNAL; }
            for (int k = 0; k < nc; k++) jobs.push_back(debwt_fm_job{p0 + r, cand[k].diag, cand[k].record, cand[k].strand});
        }
        job_first[np] = jobs.size();
        aln.resize(jobs.size());
        HIPCHK(f, hipSetDevice(f->device));
        rc = fm_extend_run(f, patterns, offsets, jobs.data(), jobs.size(), o.scoring, o.band, true, aln.data(), &cig_n, &cig);
        if (rc) return rc;
        u64 cf = pool.size();
        pool.insert(pool.end(), cig.begin(), cig.end());
        for (u64 r = 0; r < np; r++) {
            first[p0 + r] = cands.size();
            for (u64 j = job_first[r]; j < job_first[r + 1]; j++) {
                cands.push_back(FmPairCand{aln[j], jobs[j].diag, jobs[j].record, jobs[j].strand, 0u, cig_n[j], cf});
                cf += cig_n[j];
            }
        }
        p0 = p1;
    }
    first[npat] = cands.size();
    return DEBWT_OK;
}

debwt_fm_pcand fm_pair_pcand(const FmPairCand &c) {
    return debwt_fm_pcand{c.a.score, c.record, c.strand, c.rescued, c.a.tbeg, c.a.tend};
}

}  // namespace

extern "C" void debwt_fm_pair_defaults(debwt_fm_pair_opts *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    debwt_fm_map_defaults(&o->map);
    o->max_rescue = 4; o->unpaired_penalty = 17;
}

extern "C" int debwt_fm_map_pairs(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npairs,
                                  const debwt_fm_pair_opts *opts, debwt_fm_hit *hits, debwt_fm_pair_info *pairs,
                                  uint64_t *cigar_offsets, uint32_t *cigar, uint64_t capacity) {
    if (!f || !offsets || !cigar_offsets || (npairs && (!hits || !pairs)) || npairs > (1ull << 62)) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    debwt_fm_pair_opts po;
    debwt_fm_pair_defaults(&po);
    if (opts) po = *opts;
    const debwt_fm_map_opts &o = po.map;
    const u64 npat = 2 * npairs;
    f->pair_stats = debwt_fm_pair_stats{};
    f->x_stats = debwt_fm_extend_stats{};
    int rc = fm_ext_check(f, &o.scoring, o.band, "debwt_fm_map_pairs");
    if (rc) return rc;
    if (!o.min_len || !o.max_occ || !o.max_cand || o.max_cand > 4096 || o.flags) {
        f->err = "debwt_fm_map_pairs: min_len, max_occ and max_cand must be positive (max_cand <= 4096), no flag set "
                 "(pairs are mapped on both strands)";
        return DEBWT_EINVAL;
    }
    if (po.ins_lo > po.ins_hi || po.ins_hi > DEBWT_FM_INSERT_MAX) {
        f->err = "debwt_fm_map_pairs: insert bounds must be ascending and at most 16384";
        return DEBWT_EINVAL;
    }
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) { f->err = "debwt_fm_map_pairs: offsets must not decrease"; return DEBWT_EINVAL; }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    debwt_fm_pair_stats &ps = f->pair_stats;
    ps.pairs = npairs;
    const int32_t thr = std::max<int32_t>(1, o.min_score);

    // 1. the candidates of every read
    auto t = std::chrono::steady_clock::now();
    std::vector<FmPairCand> base;
    std::vector<u64> first;
    std::vector<u32> pool;
    rc = fm_pair_candidates(f, patterns, offsets, npat, o, base, first, pool);
    if (rc) return rc;
    std::vector<std::vector<debwt_fm_pcand>> pc(npat);     // what debwt_fm_pair_select reads, rescued ones appended
    std::vector<std::vector<FmPairCand>> extra(npat);      // the rescued candidates of a read
    for (u64 r = 0; r < npat; r++)
        for (u64 k = first[r]; k < first[r + 1]; k++) pc[r].push_back(fm_pair_pcand(base[k]));
    ps.ms_candidates = (float)fm_ms_since(t);

    // 2. the insert bounds
    u32 ins_lo = po.ins_lo, ins_hi = po.ins_hi;
    if (!ins_lo && !ins_hi) {
        std::vector<uint64_t> tl;
        for (u64 p = 0; p < npairs; p++) {
            const auto &a = pc[2 * p], &b = pc[2 * p + 1];
            const int32_t b1 = fm_pair_single(a.data(), (u32)a.size(), thr), b2 = fm_pair_single(b.data(), (u32)b.size(), thr);
            if (b1 < 0 || b2 < 0) continue;
            const int32_t s1 = fm_pair_sub(a.data(), (u32)a.size(), b1), s2 = fm_pair_sub(b.data(), (u32)b.size(), b2);
            if (60 * (int64_t)(a[b1].score - s1) / a[b1].score < 20 || 60 * (int64_t)(b[b2].score - s2) / b[b2].score < 20) continue;
            u64 T, tb;
            if (fm_pair_proper(a[b1], b[b2], thr, 0, DEBWT_FM_INSERT_MAX, &T, &tb)) tl.push_back(T);
        }
        ps.estimate_pairs = tl.size();
        if (debwt_fm_insert_bounds(tl.data(), tl.size(), &ins_lo, &ins_hi)) {
            f->err = "debwt_fm_map_pairs: only " + std::to_string(tl.size()) + " pairs map uniquely and face each other, " +
                     std::to_string(DEBWT_FM_INSERT_MIN_PAIRS) + " are needed to estimate the insert size: give explicit insert bounds (ins_lo, ins_hi)";
            return DEBWT_EINVAL;
        }
    }
    ps.ins_lo = ins_lo; ps.ins_hi = ins_hi;

    // 3. rescue: a window next to a candidate whose partner has no candidate that pairs with it
    t = std::chrono::steady_clock::now();
    if (po.max_rescue) {
        std::vector<debwt_fm_window_job> wj;
        std::vector<u32> ord;
        for (u64 r = 0; r < npat; r++) {
            const u64 y = r ^ 1ull, my = offsets[y + 1] - offsets[y];
            if (my < 1 || my > DEBWT_FM_WINDOW_MAX_QUERY) continue;
            const auto &cx = pc[r], &cy = pc[y];
            ord.clear();
            for (u32 k = 0; k < cx.size(); k++) if (cx[k].score >= thr) ord.push_back(k);
            std::sort(ord.begin(), ord.end(), [&](u32 a, u32 b) {
                if (cx[a].score != cx[b].score) return cx[a].score > cx[b].score;
                return std::make_tuple(cx[a].strand, cx[a].record, cx[a].tbeg, a) < std::make_tuple(cx[b].strand, cx[b].record, cx[b].tbeg, b);
            });
            if (ord.size() > po.max_rescue) ord.resize(po.max_rescue);
            const size_t w0 = wj.size();
            for (u32 k : ord) {
                const debwt_fm_pcand &c = cx[k];
                bool paired = false;
                for (const debwt_fm_pcand &d : cy) {
                    u64 T, tb;
                    if (fm_pair_proper(c, d, thr, ins_lo, ins_hi, &T, &tb)) { paired = true; break; }
                }
                if (paired) continue;
                debwt_fm_window_job jb{y, c.record, 1u - c.strand, 0, 0};
                if (c.strand == 0) { jb.wbeg = c.tbeg; jb.wend = c.tbeg + ins_hi; }
                else { jb.wbeg = c.tend > ins_hi ? c.tend - ins_hi : 0; jb.wend = c.tend; }
                bool dup = false;
                for (size_t x = w0; x < wj.size() && !dup; x++)
                    dup = wj[x].record == jb.record && wj[x].strand == jb.strand && wj[x].wbeg == jb.wbeg && wj[x].wend == jb.wend;
                if (!dup) wj.push_back(jb);
            }
        }
        ps.rescue_jobs = wj.size();
        if (!wj.empty()) {
            std::vector<debwt_fm_aln> wa(wj.size());
            std::vector<u32> cig_n, cig;
            rc = fm_window_call(f, patterns, offsets, npat, wj.data(), wj.size(), &o.scoring, true, wa.data(), &cig_n, &cig);
            if (rc) return rc;
            u64 cf = pool.size();
            pool.insert(pool.end(), cig.begin(), cig.end());
            for (size_t x = 0; x < wj.size(); cf += cig_n[x], x++) {
                const debwt_fm_aln &a = wa[x];
                if (a.score < thr) continue;
                const u64 y = wj[x].pattern;
                bool known = false;
                for (const debwt_fm_pcand &d : pc[y])
                    if (d.score > 0 && d.strand == wj[x].strand && d.tbeg == a.tbeg && d.tend == a.tend) { known = true; break; }
                if (known) continue;
                FmPairCand c{a, (int64_t)a.tbeg - (int64_t)a.qbeg, wj[x].record, wj[x].strand, 1u, cig_n[x], cf};
                extra[y].push_back(c);
                pc[y].push_back(fm_pair_pcand(c));
            }
        }
    }
    ps.ms_rescue = (float)fm_ms_since(t);

    // 4. the choice of every pair
    t = std::chrono::steady_clock::now();
    std::vector<u32> all_cig;
    cigar_offsets[0] = 0;
    for (u64 p = 0; p < npairs; p++) {
        debwt_fm_pair_choice ch;
        rc = debwt_fm_pair_select(pc[2 * p].data(), (u32)pc[2 * p].size(), pc[2 * p + 1].data(), (u32)pc[2 * p + 1].size(),
                                  ins_lo, ins_hi, po.unpaired_penalty, o.min_score, &ch);
        if (rc) { f->err = "debwt_fm_map_pairs: a candidate with an empty text interval"; return DEBWT_EINTERNAL; }
        pairs[p] = debwt_fm_pair_info{ch.tlen, ch.pair_score, ch.pair_sub, 0u};
        ps.proper += ch.proper;
        for (u32 x = 0; x < 2; x++) {
            const u64 r = 2 * p + x, m = offsets[r + 1] - offsets[r];
            const int32_t w = x ? ch.i2 : ch.i1;
            debwt_fm_hit &h = hits[r];
            memset(&h, 0, sizeof h);
            h.pattern = r;
            h.flags = DEBWT_FM_MAP_UNMAPPED | (m > FM_EXT_MAX_LEN ? DEBWT_FM_MAP_TOO_LONG : 0u);
            cigar_offsets[r + 1] = cigar_offsets[r];
            if (w < 0) continue;
            const u64 nbase = first[r + 1] - first[r];
            const FmPairCand &c = (u64)w < nbase ? base[first[r] + w] : extra[r][w - nbase];
            const debwt_fm_aln &a = c.a;
            h.flags = (c.strand ? DEBWT_FM_MAP_REVERSE : 0u) | (ch.proper ? DEBWT_FM_MAP_PROPER : 0u) |
                      (c.rescued ? DEBWT_FM_MAP_RESCUED : 0u);
            h.record = c.record; h.offset = a.tbeg - f->rec_starts[c.record];
            h.qbeg = a.qbeg; h.qend = a.qend; h.tbeg = a.tbeg; h.tend = a.tend;
            h.score = a.score; h.sub = x ? ch.sub2 : ch.sub1; h.mapq = x ? ch.mapq2 : ch.mapq1; h.edits = a.edits;
            h.diag = c.diag;
            all_cig.insert(all_cig.end(), pool.begin() + c.cig_first, pool.begin() + c.cig_first + c.cig_n);
            cigar_offsets[r + 1] = all_cig.size();
            ps.rescued += c.rescued;
        }
    }
    ps.ms_select = (float)fm_ms_since(t);
    ps.ms_wall = (float)fm_ms_since(t0);
    if (capacity < all_cig.size() || (!all_cig.empty() && !cigar)) {
        f->err = "debwt_fm_map_pairs: capacity below the CIGAR ops (cigar_offsets[2 npairs] = " + std::to_string(all_cig.size()) + ")";
        return DEBWT_ERANGE;
    }
    if (!all_cig.empty()) memcpy(cigar, all_cig.data(), all_cig.size() * 4);
    return DEBWT_OK;
}

extern "C" int debwt_fm_pair_stats_get(const debwt_fm *f, debwt_fm_pair_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->pair_stats;
    return DEBWT_OK;
}

// ---- extract and text restore (fm_extract_kernels.h) ----------------------------------------------------------------
// The anchors are made by the first call that needs them and stay with the index.  An extract batch is planned on the
// device (per job the anchor gaps that meet it), laid out by a prefix sum on the host and walked one gap per item, so a
// job of 10^6 bases is 10^6 / s items, not one lane's walk.  A restore walks every gap once into the packed text.

namespace {

constexpr u64 FM_EXTRACT_BYTES = 256ull << 20;         // output bytes of one extract batch
constexpr u64 FM_EXTRACT_JOBS = 1ull << 22;            // jobs of one extract batch

FmAnchors fm_anchors_of(const debwt_fm *f) {
    return FmAnchors{f->anchors.as<u64>(), f->sa.as<u64>(), f->na, f->nsamp, f->sh};
}

int fm_anchors_build(debwt_fm *f) {
    if (f->has_anchors) return DEBWT_OK;
    const u64 n = f->n, nsamp = f->nsamp;
    const u64 nwords = (n + 63) >> 6, nchunks = (nwords + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;
    FmTmp bits, wpre, csum;
    HIPCHK(f, hipMalloc(&bits.p, (size_t)nwords * 8));
    HIPCHK(f, hipMalloc(&wpre.p, (size_t)nwords * 4));
    HIPCHK(f, hipMalloc(&csum.p, (size_t)nchunks * 8));
    FM_ENSURE(f, f->e_ctr, 64);
    u64 *ctr = f->e_ctr.as<u64>(), *d_bits = reinterpret_cast<u64 *>(bits.p);
    HIPCHK(f, hipMemsetAsync(d_bits, 0, (size_t)nwords * 8, f->stream));
    HIPCHK(f, hipMemsetAsync(ctr, 0, 64, f->stream));
    hipEvent_t e0, e1;
    HIPCHK(f, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); f->err = "hipEventCreate"; return DEBWT_EDEVICE; }
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    (void)hipEventRecord(e0, f->stream);
    k_fm_anc_mark<<<grid_for(nsamp, 256), 256, 0, f->stream>>>(f->sa.as<u64>(), nsamp, n, d_bits, ctr);
    k_fm_anc_free<<<1, 64, 0, f->stream>>>(n, d_bits, ctr);
    u64 h[8];
    HIPCHK(f, hipMemcpyAsync(h, ctr, 64, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    if (h[FM_EX_A_RANGE] || h[FM_EX_A_DUP]) {
        f->err = "the samples are not a suffix array of the rows: " + std::to_string(h[FM_EX_A_RANGE]) +
                 " are no text position, " + std::to_string(h[FM_EX_A_DUP]) + " repeat another sample's position";
        return DEBWT_EINVAL;
    }
    const u64 na = nsamp + h[FM_EX_A_FIRST] + h[FM_EX_A_LAST];
    FM_ENSURE(f, f->anchors, (size_t)na * 8);
    HIPCHK(f, hipMemsetAsync(f->anchors.p, 0xFF, (size_t)na * 8, f->stream));
    k_fm_anc_count<<<(u32)nchunks, FM_EX_CHUNK_WORDS, 0, f->stream>>>(d_bits, nwords, reinterpret_cast<u32 *>(wpre.p),
                                                                     reinterpret_cast<u64 *>(csum.p));
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(reinterpret_cast<u64 *>(csum.p), nchunks, ctr + FM_EX_A_TOTAL);
    k_fm_anc_scatter<<<grid_for(nsamp + 2, 256), 256, 0, f->stream>>>(f->sa.as<u64>(), nsamp, n, d_bits,
                                                                     reinterpret_cast<const u32 *>(wpre.p),
                                                                     reinterpret_cast<const u64 *>(csum.p), ctr, na,
                                                                     f->anchors.as<u64>());
    (void)hipEventRecord(e1, f->stream);
    HIPCHK(f, hipMemcpyAsync(h, ctr, 64, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    if (h[FM_EX_A_TOTAL] != na) { f->err = "anchors: the rank over the sampled positions is inconsistent"; return DEBWT_EINTERNAL; }
    (void)hipEventElapsedTime(&f->ms_anchors, e0, e1);
    f->na = na;
    f->has_anchors = true;
    return DEBWT_OK;
}

// one walk over nitems items; the counters come back in h[0..7] and are added to the stats
template <class E>
int fm_extract_walk(debwt_fm *f, const E &em, u64 nitems, bool pad, u64 h[8]) {
    debwt_fm_extract_stats &st = f->e_stats;
    u64 *ctr = f->e_ctr.as<u64>();
    hipEvent_t e0, e1;
    HIPCHK(f, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); f->err = "hipEventCreate"; return DEBWT_EDEVICE; }
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    // a run per wave long enough that the drain of its last items is a small part of it, short enough for several
    // waves per SIMD slot of the device
    const u32 chunk = (u32)std::min<u64>(std::max<u64>(nitems / 16384, 128), 4096);
    const u64 waves = (nitems + chunk - 1) / chunk;
    HIPCHK(f, hipMemsetAsync(ctr, 0, 64, f->stream));
    (void)hipEventRecord(e0, f->stream);
    k_fm_extract_walk<E><<<grid_for(waves * 64, 256), 256, 0, f->stream>>>(f->V, fm_anchors_of(f), em, nitems, chunk, ctr);
    if (pad) k_fm_extract_pad<<<1, 64, 0, f->stream>>>(f->text.as<u64>(), f->n);
    (void)hipEventRecord(e1, f->stream);
    HIPCHK(f, hipMemcpyAsync(h, ctr, 64, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    st.ms_kernel += ms; st.launches += pad ? 2 : 1; st.segments += nitems;
    st.steps += h[FM_EX_W_STEPS]; st.line_reads += h[FM_EX_W_STEPS]; st.wave_steps += h[FM_EX_W_WAVE];
    return DEBWT_OK;
}

int fm_extract_begin(debwt_fm *f) {
    f->e_stats = debwt_fm_extract_stats{};
    HIPCHK(f, hipSetDevice(f->device));
    const bool had = f->has_anchors;
    int rc = fm_anchors_build(f);
    if (rc) return rc;
    f->e_stats.anchor_bytes = f->anchors.cap;
    f->e_stats.ms_anchors = had ? 0.f : f->ms_anchors;
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_extract(debwt_fm *f, const debwt_fm_extract_job *jobs, uint64_t njobs, uint64_t *out_offsets,
                                char *bases, uint64_t capacity) {
    if (!f || !out_offsets || (njobs && !jobs)) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->e_stats = debwt_fm_extract_stats{};
    const u64 n = f->n, nrec = f->nrec;
    const std::vector<u64> &rs = f->rec_starts;
    out_offsets[0] = 0;
    for (u64 j = 0; j < njobs; j++) {
        const debwt_fm_extract_job &q = jobs[j];
        if (q.reserved) { f->err = "debwt_fm_extract: job " + std::to_string(j) + " has a non-zero reserved field"; return DEBWT_EINVAL; }
        if (q.record >= nrec) { f->err = "debwt_fm_extract: job " + std::to_string(j) + " names record " + std::to_string(q.record) + " of " + std::to_string(nrec); return DEBWT_EINVAL; }
        const u64 len = (q.record + 1 < nrec ? rs[q.record + 1] : n) - 1 - rs[q.record];
        if (q.offset > len) { f->err = "debwt_fm_extract: job " + std::to_string(j) + " begins at " + std::to_string(q.offset) + " in a record of " + std::to_string(len) + " bases"; return DEBWT_EINVAL; }
        out_offsets[j + 1] = out_offsets[j] + std::min<u64>(q.length, len - q.offset);
    }
    const u64 total = out_offsets[njobs];
    f->e_stats.jobs = njobs; f->e_stats.bases = total;
    if (capacity < total || (total && !bases)) {
        f->err = "debwt_fm_extract: capacity below the bases asked for (out_offsets[njobs] = " + std::to_string(total) + ")";
        return DEBWT_ERANGE;
    }
    if (!total) return DEBWT_OK;
    int rc = fm_extract_begin(f);
    if (rc) return rc;
    f->e_stats.jobs = njobs; f->e_stats.bases = total;
    const u64 limit = fm_env_u64("DEBWT_FM_EXTRACT_BYTES", FM_EXTRACT_BYTES);
    std::vector<FmExJob> hj;
    std::vector<u64> seg;
    for (u64 j0 = 0; j0 < njobs;) {
        u64 j1 = j0 + 1;                                       // at least one job, however long
        while (j1 < njobs && j1 - j0 < FM_EXTRACT_JOBS && out_offsets[j1 + 1] - out_offsets[j0] <= limit) j1++;
        const u64 nb = j1 - j0, bytes = out_offsets[j1] - out_offsets[j0];
        if (!bytes) { j0 = j1; continue; }
        hj.resize(nb); seg.resize(nb + 1);
        for (u64 j = 0; j < nb; j++) {
            const debwt_fm_extract_job &q = jobs[j0 + j];
            const u64 a = rs[q.record] + q.offset;
            hj[j] = FmExJob{a, a + (out_offsets[j0 + j + 1] - out_offsets[j0 + j]), out_offsets[j0 + j] - out_offsets[j0], 0};
        }
        FM_ENSURE(f, f->e_jobs, (size_t)nb * sizeof(FmExJob));
        FM_ENSURE(f, f->e_seg, (size_t)(nb + 1) * 8);
        FM_ENSURE(f, f->e_out, (size_t)bytes);
        HIPCHK(f, hipMemcpyAsync(f->e_jobs.p, hj.data(), nb * sizeof(FmExJob), hipMemcpyHostToDevice, f->stream));
        k_fm_extract_plan<<<grid_for(nb, 256), 256, 0, f->stream>>>(f->V, fm_anchors_of(f), f->e_jobs.as<FmExJob>(), nb,
                                                                    f->e_seg.as<u64>());
        HIPCHK(f, hipMemcpyAsync(seg.data(), f->e_seg.p, nb * 8, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
        f->e_stats.launches++;
        u64 run = 0;
        for (u64 j = 0; j < nb; j++) { const u64 c = seg[j]; seg[j] = run; run += c; }
        seg[nb] = run;
        HIPCHK(f, hipMemcpyAsync(f->e_seg.p, seg.data(), (nb + 1) * 8, hipMemcpyHostToDevice, f->stream));
        u64 h[8];
        const FmExAscii em{f->e_jobs.as<FmExJob>(), f->e_seg.as<u64>(), nb, f->e_out.as<u8>()};
        if ((rc = fm_extract_walk(f, em, run, false, h))) return rc;
        if (h[FM_EX_W_CHAIN] || h[FM_EX_W_BAD]) {
            f->err = "debwt_fm_extract: the samples are not those of the rows (" + std::to_string(h[FM_EX_W_CHAIN]) +
                     " walks missed the row of their anchor, " + std::to_string(h[FM_EX_W_BAD]) + " left their record)";
            return DEBWT_EINVAL;
        }
        HIPCHK(f, hipMemcpyAsync(bases + out_offsets[j0], f->e_out.p, bytes, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
        f->e_stats.batches++;
        j0 = j1;
    }
    f->e_stats.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_extract_stats_get(const debwt_fm *f, debwt_fm_extract_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->e_stats;
    return DEBWT_OK;
}

extern "C" int debwt_fm_restore_text(debwt_fm *f) {
    if (!f) return DEBWT_EINVAL;
    if (f->has_text) return DEBWT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = fm_extract_begin(f);
    if (rc) return rc;
    debwt_fm_extract_stats &st = f->e_stats;
    const u64 n = f->n, nrec = f->nrec;
    const size_t tw = (size_t)((n + 63) >> 5) + 2;
    FM_ENSURE(f, f->text, tw * 8);
    FM_ENSURE(f, f->e_sep, (size_t)nrec * 8);
    FM_ENSURE(f, f->s_ctr, 64);
    HIPCHK(f, hipMemsetAsync(f->text.p, 0, tw * 8, f->stream));
    u64 h[8];
    const FmExPacked em{f->text.as<u64>(), f->e_sep.as<u64>(), nrec};
    if ((rc = fm_extract_walk(f, em, f->na - 1, true, h))) return rc;
    st.bases = n; st.batches = 1;
    if (h[FM_EX_W_CHAIN] || h[FM_EX_W_BAD] || h[FM_EX_W_STEPS] != n - 1 || h[FM_EX_W_SEPS] != nrec - 1) {
        f->err = "debwt_fm_restore_text: the samples are not those of the rows (" + std::to_string(h[FM_EX_W_CHAIN]) +
                 " segments missed the row of their lower anchor or the '$' at the text's start, " +
                 std::to_string(h[FM_EX_W_BAD]) + " were refused, " + std::to_string(h[FM_EX_W_SEPS]) + " separators met, " +
                 std::to_string(nrec - 1) + " expected)";
        return DEBWT_EINVAL;
    }
    std::vector<u64> sp(nrec - 1);
    if (nrec > 1) {
        HIPCHK(f, hipMemcpyAsync(sp.data(), f->e_sep.p, (nrec - 1) * 8, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
        std::sort(sp.begin(), sp.end());
    }
    for (u64 r = 0; r + 1 < nrec; r++)
        if (sp[r] != f->rec_starts[r + 1] - 1) {               // a '$' met inside the text carries bit 63: never equal
            f->err = "debwt_fm_restore_text: separator " + std::to_string(r) + " was met at " + std::to_string(sp[r] & ~(1ull << 63)) +
                     ", the index has it at " + std::to_string(f->rec_starts[r + 1] - 1);
            return DEBWT_EINVAL;
        }
    HIPCHK(f, hipMemsetAsync(f->s_ctr.p, 0, 8, f->stream));
    k_fm_text_check<<<grid_for(f->nsamp, 256), 256, 0, f->stream>>>(f->V, f->sa.as<u64>(), f->nsamp, f->sh, f->text.as<u64>(),
                                                                   f->s_ctr.as<u64>());
    u64 bad = 0;
    HIPCHK(f, hipMemcpyAsync(&bad, f->s_ctr.p, 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    st.launches++;
    if (bad) {
        f->err = "debwt_fm_restore_text: the restored text fails the check of debwt_fm_attach_text (" + std::to_string(bad) +
                 " of " + std::to_string(f->nsamp) + " sampled rows)";
        return DEBWT_EINVAL;
    }
    f->has_text = true;
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_text_fetch(debwt_fm *f, uint64_t *packed, uint64_t capacity_words, uint64_t *sep) {
    if (!f || !packed || !sep) return DEBWT_EINVAL;
    if (!f->has_text) { f->err = "debwt_fm_text_fetch: no text attached (debwt_fm_attach_text, debwt_fm_restore_text)"; return DEBWT_ESTATE; }
    const u64 n = f->n, nrec = f->nrec, tw = ((n + 63) >> 5) + 2;
    if (capacity_words < tw) { f->err = "debwt_fm_text_fetch: capacity below ((n + 63) >> 5) + 2 = " + std::to_string(tw) + " words"; return DEBWT_ERANGE; }
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipMemcpyAsync(packed, f->text.p, (size_t)tw * 8, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    for (u64 r = 0; r < nrec; r++) sep[r] = (r + 1 < nrec ? f->rec_starts[r + 1] : n) - 1;
    return DEBWT_OK;
}

// ---- k-mer counts along reads and read correction (fm_kmer_kernels.h) ------------------------------------------------
// A batch of patterns [p0, p1) runs as one lane per (position, strand); the positions of the batch are numbered by the
// prefix sums of the reads' k-mer numbers, which the kernels search for the read of a lane.  The prefix table is made by
// the first call that wants it and kept.  The correction keeps a batch's reads in q_chars over all its rounds: profile,
// trials, evaluation and fixes are kernels, and per round only the number of reads that got a fix comes back.

namespace {

constexpr u64 FM_KMER_ITEMS = 1ull << 24;              // k-mer positions per batch
constexpr u32 FM_KMER_TABLE_Q = 12;                    // default q of the prefix table

int fm_kmer_env_q(debwt_fm *f, u32 *q) {
    *q = FM_KMER_TABLE_Q;
    const char *e = getenv("DEBWT_FM_KMER_TABLE_Q");
    if (!e || !*e) return DEBWT_OK;
    char *end = nullptr;
    const u64 v = strtoull(e, &end, 10);
    if (*end || v > FM_KMER_MAX_Q) { f->err = "DEBWT_FM_KMER_TABLE_Q must be 0..12"; return DEBWT_EINVAL; }
    *q = (u32)v;
    return DEBWT_OK;
}

// the table of q-mers in f->k_table (q >= 1): kept when it is there, otherwise built level by level (st->ms_table)
int fm_kmer_table(debwt_fm *f, u32 q, debwt_fm_kmer_stats *st) {
    st->table_q = q;
    if (!q || (f->has_ktable && f->k_q == q)) return DEBWT_OK;
    const size_t bytes = (size_t)16 << (2 * q);
    f->has_ktable = false;
    if (f->k_table.cap != bytes) {                            // exactly the table: it is reported in device_bytes
        HIPCHK(f, hipStreamSynchronize(f->stream));
        if (f->k_table.p) { (void)hipFree(f->k_table.p); f->k_table.p = nullptr; f->k_table.cap = 0; }
        HIPCHK(f, hipMalloc(&f->k_table.p, bytes));
        f->k_table.cap = bytes;
    }
    hipEvent_t e0, e1;
    HIPCHK(f, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); f->err = "hipEventCreate"; return DEBWT_EDEVICE; }
    struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev{e0, e1};
    const u64 root[2] = {0, f->n};
    HIPCHK(f, hipMemcpyAsync(f->k_table.p, root, 16, hipMemcpyHostToDevice, f->stream));
    (void)hipEventRecord(e0, f->stream);
    for (u32 l = 1; l <= q; l++) {
        const u64 prev = 1ull << (2 * (l - 1));
        k_fm_kmer_table_level<<<grid_for(prev, 256), 256, 0, f->stream>>>(f->V, f->k_table.as<u64>(), prev);
        st->launches++;
    }
    (void)hipEventRecord(e1, f->stream);
    int rc = fm_sync(f);                                       // root is host memory
    if (rc) return rc;
    (void)hipEventElapsedTime(&st->ms_table, e0, e1);
    f->has_ktable = true;
    f->k_q = q;
    return DEBWT_OK;
}

struct FmKmerCall {                                     // what kmer_counts and correct share
    u32 k = 0, nstr = 1, q = 0;
    u64 limit = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~FmKmerCall() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

inline u64 fm_kmer_nk(const uint64_t *offsets, u64 i, u32 k) {
    const u64 m = offsets[i + 1] - offsets[i];
    return m >= k ? m - k + 1 : 0;
}

int fm_kmer_begin(debwt_fm *f, const char *what, const char *patterns, const uint64_t *offsets, u64 npat, u32 k, u32 flags,
                  u64 max_len, FmKmerCall *c, debwt_fm_kmer_stats *st) {
    if (!k) { f->err = std::string(what) + ": k must be at least 1"; return DEBWT_EINVAL; }
    if (flags & ~DEBWT_FM_BOTH_STRANDS) { f->err = std::string(what) + ": unknown flags"; return DEBWT_EINVAL; }
    for (u64 i = 0; i < npat; i++) {
        if (offsets[i + 1] < offsets[i]) { f->err = std::string(what) + ": offsets must not decrease"; return DEBWT_EINVAL; }
        if (offsets[i + 1] - offsets[i] >= max_len) { f->err = std::string(what) + ": a pattern is too long"; return DEBWT_EINVAL; }
    }
    if (npat && offsets[npat] > offsets[0] && !patterns) return DEBWT_EINVAL;
    int rc = fm_kmer_env_q(f, &c->q);
    if (rc) return rc;
    if (k < c->q) c->q = 0;                                    // every k-mer walks from [0, n): the call needs no table
    c->k = k;
    c->nstr = (flags & DEBWT_FM_BOTH_STRANDS) ? 2 : 1;
    c->limit = fm_env_u64("DEBWT_FM_KMER_ITEMS", FM_KMER_ITEMS);
    st->patterns = npat;
    if (!npat) return DEBWT_OK;
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipEventCreate(&c->e0));
    HIPCHK(f, hipEventCreate(&c->e1));
    if ((rc = fm_kmer_table(f, c->q, st))) return rc;
    FM_ENSURE(f, f->k_ctr, FM_KM_NCTR * 8);
    HIPCHK(f, hipMemsetAsync(f->k_ctr.p, 0, FM_KM_NCTR * 8, f->stream));
    return DEBWT_OK;
}

// end of the batch that begins at p0: at least one pattern, however long
u64 fm_kmer_cut(const uint64_t *offsets, u64 npat, u64 p0, const FmKmerCall &c, u64 *items) {
    u64 p1 = p0 + 1, it = fm_kmer_nk(offsets, p0, c.k);
    while (p1 < npat && p1 - p0 < FM_BATCH_PATTERNS && offsets[p1 + 1] - offsets[p0] <= FM_BATCH_CHARS &&
           it + fm_kmer_nk(offsets, p1, c.k) <= c.limit)
        it += fm_kmer_nk(offsets, p1++, c.k);
    *items = it;
    return p1;
}

// the batch's bytes, offsets and position numbers to q_chars, q_off and k_coff
int fm_kmer_upload(debwt_fm *f, const char *patterns, const uint64_t *offsets, u64 p0, u64 p1, u32 k, u64 items) {
    const u64 np = p1 - p0, base = offsets[p0], bytes = offsets[p1] - base;
    std::vector<u64> coff(np + 1);
    coff[0] = 0;
    for (u64 i = 0; i < np; i++) coff[i + 1] = coff[i] + fm_kmer_nk(offsets, p0 + i, k);
    FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(bytes, 1));
    FM_ENSURE(f, f->q_off, (size_t)(np + 1) * 8);
    FM_ENSURE(f, f->k_coff, (size_t)(np + 1) * 8);
    FM_ENSURE(f, f->k_counts, (size_t)std::max<u64>(items, 1) * 4);
    if (bytes) HIPCHK(f, hipMemcpyAsync(f->q_chars.p, patterns + base, bytes, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->q_off.p, offsets + p0, (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->k_coff.p, coff.data(), (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
    return fm_sync(f);                                         // coff is host memory
}

void fm_kmer_profile_launch(debwt_fm *f, const FmKmerCall &c, u64 base, u64 np, u64 items, const u8 *active,
                            debwt_fm_kmer_stats *st) {
    k_fm_kmer_profile<<<grid_for(items * c.nstr, 256), 256, 0, f->stream>>>(
        f->V, c.q ? f->k_table.as<u64>() : nullptr, c.q, f->q_chars.as<u8>(), f->q_off.as<u64>(), base, f->k_coff.as<u64>(), np,
        items, c.k, c.nstr, active, f->k_counts.as<u32>(), f->k_ctr.as<u64>());
    st->launches++;
}

int fm_kmer_end(debwt_fm *f, debwt_fm_kmer_stats *st, u64 h[FM_KM_NCTR]) {
    HIPCHK(f, hipMemcpyAsync(h, f->k_ctr.p, FM_KM_NCTR * 8, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    st->steps = h[FM_KM_STEPS]; st->line_reads = h[FM_KM_READS]; st->wave_steps = h[FM_KM_WSTEPS];
    st->table_starts = h[FM_KM_TSTART]; st->kmers = h[FM_KM_KMERS];
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_kmer_counts(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat, uint32_t k,
                                    uint32_t flags, uint64_t *count_offsets, uint32_t *counts, uint64_t capacity) {
    if (!f || !offsets || !count_offsets) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->k_stats = debwt_fm_kmer_stats{};
    debwt_fm_kmer_stats &st = f->k_stats;
    FmKmerCall c;
    int rc = fm_kmer_begin(f, "debwt_fm_kmer_counts", patterns, offsets, npat, k, flags, 1ull << 32, &c, &st);
    if (rc) return rc;
    count_offsets[0] = 0;
    for (u64 i = 0; i < npat; i++) count_offsets[i + 1] = count_offsets[i] + fm_kmer_nk(offsets, i, k);
    const u64 total = count_offsets[npat];
    if (capacity < total || (total && !counts)) {
        f->err = "debwt_fm_kmer_counts: capacity below the k-mers (count_offsets[npat] = " + std::to_string(total) + ")";
        return DEBWT_ERANGE;
    }
    for (u64 p0 = 0; p0 < npat;) {
        u64 items;
        const u64 p1 = fm_kmer_cut(offsets, npat, p0, c, &items);
        if (items) {
            const u64 np = p1 - p0;
            if ((rc = fm_kmer_upload(f, patterns, offsets, p0, p1, k, items))) return rc;
            st.scratch_bytes = std::max<u64>(st.scratch_bytes, (offsets[p1] - offsets[p0]) + (np + 1) * 16 + items * 4);
            (void)hipEventRecord(c.e0, f->stream);
            fm_kmer_profile_launch(f, c, offsets[p0], np, items, nullptr, &st);
            (void)hipEventRecord(c.e1, f->stream);
            HIPCHK(f, hipMemcpyAsync(counts + count_offsets[p0], f->k_counts.p, items * 4, hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;                  // the next batch reuses the scratch
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, c.e0, c.e1);
            st.ms_kernel += ms;
        }
        st.batches++;
        p0 = p1;
    }
    u64 h[FM_KM_NCTR];
    if (npat && (rc = fm_kmer_end(f, &st, h))) return rc;
    st.ms_wall = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DEBWT_OK;
}

extern "C" int debwt_fm_kmer_stats_get(const debwt_fm *f, debwt_fm_kmer_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->k_stats;
    return DEBWT_OK;
}

extern "C" int debwt_fm_weak_trials(const uint32_t *counts, uint64_t nk, uint32_t k, uint32_t min_count, debwt_fm_trial *out,
                                    uint64_t capacity) {
    if (!k || !min_count || nk + k > (1ull << 31) || (nk && !counts) || (capacity && !out)) return DEBWT_EINVAL;
    u64 n = 0;
    fm_weak_trials(counts, (u32)nk, k, min_count, [&](u32 a, u32 b, u32 pos, u32 window, u32 kind) {
        if (n < capacity) out[n] = debwt_fm_trial{a, b, pos, window, kind};
        n++;
    });
    return (int)n;
}

extern "C" void debwt_fm_correct_defaults(debwt_fm_correct_opts *o) {
    if (!o) return;
    o->k = 0; o->min_count = 3; o->max_rounds = 4; o->flags = DEBWT_FM_BOTH_STRANDS;
}

extern "C" int debwt_fm_correct(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                                const debwt_fm_correct_opts *opts, char *out, debwt_fm_correct_info *info) {
    if (!f || !offsets || !opts || (npat && !info)) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->c_stats = debwt_fm_correct_stats{};
    debwt_fm_correct_stats &cs = f->c_stats;
    debwt_fm_kmer_stats &st = cs.kmers;
    const u32 k = opts->k, min_count = opts->min_count, rounds = opts->max_rounds;
    if (!min_count) { f->err = "debwt_fm_correct: min_count must be at least 1"; return DEBWT_EINVAL; }
    if (rounds < 1 || rounds > DEBWT_FM_CORRECT_MAX_ROUNDS) { f->err = "debwt_fm_correct: max_rounds must be 1..16"; return DEBWT_EINVAL; }
    FmKmerCall c;
    int rc = fm_kmer_begin(f, "debwt_fm_correct", patterns, offsets, npat, k, opts->flags, 1ull << 31, &c, &st);
    if (rc) return rc;
    if (npat && offsets[npat] > offsets[0] && !out) return DEBWT_EINVAL;
    std::vector<u8> act;
    for (u64 p0 = 0; p0 < npat;) {
        u64 items;
        const u64 p1 = fm_kmer_cut(offsets, npat, p0, c, &items);
        const u64 np = p1 - p0, base = offsets[p0], bytes = offsets[p1] - base, nslots = items + np;
        debwt_fm_correct_info *inf = info + p0;
        memset(inf, 0, np * sizeof *inf);
        if (!items) {                                          // short reads only: copied
            if (bytes) memcpy(out + base, patterns + base, bytes);
        } else {
            if ((rc = fm_kmer_upload(f, patterns, offsets, p0, p1, k, items))) return rc;
            FM_ENSURE(f, f->k_active, (size_t)np);
            FM_ENSURE(f, f->k_info, (size_t)np * 16);
            FM_ENSURE(f, f->k_ntr, (size_t)np * 4);
            FM_ENSURE(f, f->k_trials, (size_t)nslots * 8);
            FM_ENSURE(f, f->k_trun, (size_t)nslots * 4);
            FM_ENSURE(f, f->k_res, (size_t)nslots);
            st.scratch_bytes = std::max<u64>(st.scratch_bytes, bytes + (np + 1) * 16 + items * 4 + np * 21 + nslots * 13);
            act.resize(np);
            for (u64 i = 0; i < np; i++) act[i] = fm_kmer_nk(offsets, p0 + i, k) ? 1 : 0;
            HIPCHK(f, hipMemcpyAsync(f->k_active.p, act.data(), np, hipMemcpyHostToDevice, f->stream));
            HIPCHK(f, hipMemsetAsync(f->k_info.p, 0, np * 16, f->stream));
            u8 *d_act = f->k_active.as<u8>();
            u64 *ctr = f->k_ctr.as<u64>();
            for (u32 r = 0; r <= rounds; r++) {
                const bool last = r == rounds;                 // after the last round: the profile of weak_after alone
                (void)hipEventRecord(c.e0, f->stream);
                fm_kmer_profile_launch(f, c, base, np, items, d_act, &st);
                k_fm_correct_trials<<<grid_for(np, 256), 256, 0, f->stream>>>(
                    f->k_coff.as<u64>(), np, k, min_count, f->k_counts.as<u32>(), d_act, r == 0, last, f->k_trials.as<u32>(),
                    f->k_trun.as<u32>(), f->k_ntr.as<u32>(), f->k_info.as<u32>(), ctr);
                st.launches++;
                u64 got = 0;
                if (!last) {
                    HIPCHK(f, hipMemsetAsync(ctr + FM_KM_ACTIVE, 0, 8, f->stream));
                    k_fm_correct_eval<<<grid_for(nslots * 4 * c.nstr, 256), 256, 0, f->stream>>>(
                        f->V, c.q ? f->k_table.as<u64>() : nullptr, c.q, f->q_chars.as<u8>(), f->q_off.as<u64>(), base,
                        f->k_coff.as<u64>(), np, nslots, k, c.nstr, min_count, d_act, f->k_trials.as<u32>(),
                        f->k_ntr.as<u32>(), f->k_res.as<u8>(), ctr);
                    k_fm_correct_apply<<<grid_for(np, 256), 256, 0, f->stream>>>(
                        f->q_chars.as<u8>(), f->q_off.as<u64>(), base, f->k_coff.as<u64>(), np, f->k_trials.as<u32>(),
                        f->k_trun.as<u32>(), f->k_ntr.as<u32>(), f->k_res.as<u8>(), d_act, f->k_info.as<u32>(), ctr);
                    st.launches += 2;
                    HIPCHK(f, hipMemcpyAsync(&got, ctr + FM_KM_ACTIVE, 8, hipMemcpyDeviceToHost, f->stream));
                }
                (void)hipEventRecord(c.e1, f->stream);
                if ((rc = fm_sync(f))) return rc;
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, c.e0, c.e1);
                st.ms_kernel += ms;
                if (last) { cs.ms_round[rounds - 1] += ms; break; }
                cs.ms_round[r] += ms;
                cs.active[r] += got;
                cs.rounds = std::max<u64>(cs.rounds, r + 1);
                if (!got) break;
            }
            if (bytes) HIPCHK(f, hipMemcpyAsync(out + base, f->q_chars.p, bytes, hipMemcpyDeviceToHost, f->stream));
            HIPCHK(f, hipMemcpyAsync(inf, f->k_info.p, np * 16, hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;                  // the next batch reuses the scratch
        }
        for (u64 i = 0; i < np; i++) {
            debwt_fm_correct_info &x = inf[i];
            if (!fm_kmer_nk(offsets, p0 + i, k)) { x = debwt_fm_correct_info{DEBWT_FM_CORRECT_SHORT, 0, 0, 0}; cs.reads_short++; }
            else if (!x.weak_before) { x.flags = DEBWT_FM_CORRECT_CLEAN; cs.reads_clean++; }
            else if (!x.weak_after) { x.flags = DEBWT_FM_CORRECT_FIXED; cs.reads_fixed++; }
            else { x.flags = DEBWT_FM_CORRECT_WEAK; cs.reads_weak++; }
        }
        st.batches++;
        p0 = p1;
    }
    u64 h[FM_KM_NCTR] = {};
    if (npat && (rc = fm_kmer_end(f, &st, h))) return rc;
    cs.trials = h[FM_KM_TRIALS]; cs.fixes = h[FM_KM_FIXES];
    st.ms_wall = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DEBWT_OK;
}

extern "C" int debwt_fm_correct_stats_get(const debwt_fm *f, debwt_fm_correct_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->c_stats;
    return DEBWT_OK;
}

// ---- k-mer spectrum of the indexed collection (fm_spectrum_kernels.h) --------------------------------------------------
// The start entries (table order) are cut into chunks on the host from the sums of 1024-entry granules, which a sizing
// kernel makes per call; only a granule that a cut falls into is fetched.  A chunk is a run of launches without a host
// round trip: cursors cleared, start, one expansion per level over the chunk's bound, leaves.  The histogram and the
// totals stay on the device until the end; list members are staged on the device and flushed when the staging could
// overflow, then sorted on the host.

namespace {

constexpr u64 FM_SPECTRUM_ITEMS = 1ull << 22;          // sum of hi - lo over the start entries of a chunk: 192 MiB of frontiers
constexpr u64 FM_SPECTRUM_STAGE = 1ull << 16;          // least list staging (members), so small chunks do not flush one by one

struct FmSpecChunk { u64 i0, i1, sum, entries; };

// chunks of the table's entries [0, 4^q): runs of entries whose sizes sum to at most limit; an entry above it goes alone
int fm_spectrum_plan(debwt_fm *f, u32 q, u64 limit, std::vector<FmSpecChunk> *chunks, debwt_fm_spectrum_stats *st) {
    if (!q) { chunks->push_back(FmSpecChunk{0, 1, f->n, 1}); return DEBWT_OK; }
    const u64 T = 1ull << (2 * q), G = FM_SPEC_GRANULE, ng = (T + G - 1) / G;
    FM_ENSURE(f, f->sp_gsum, (size_t)ng * 16);
    k_fm_spectrum_sizes<<<(u32)ng, 256, 0, f->stream>>>(f->k_table.as<u64>(), T, f->sp_gsum.as<u64>());
    st->launches++;
    std::vector<u64> gs(2 * ng), gran(2 * G);
    HIPCHK(f, hipMemcpyAsync(gs.data(), f->sp_gsum.p, (size_t)ng * 16, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    u64 loaded = ~0ull;
    for (u64 i = 0; i < T;) {
        FmSpecChunk c{i, i, 0, 0};
        while (i < T) {
            const u64 g = i / G;
            if (i % G == 0 && c.sum + gs[2 * g] <= limit) {     // the whole granule fits
                c.sum += gs[2 * g]; c.entries += gs[2 * g + 1];
                i = std::min<u64>(T, i + G);
                if (c.sum >= limit) break;
                continue;
            }
            if (loaded != g) {
                const u64 cnt = std::min<u64>(G, T - g * G);
                HIPCHK(f, hipMemcpyAsync(gran.data(), f->k_table.as<u64>() + 2 * g * G, (size_t)cnt * 16, hipMemcpyDeviceToHost, f->stream));
                if ((rc = fm_sync(f))) return rc;
                loaded = g;
            }
            const u64 lo = gran[2 * (i - g * G)], hi = gran[2 * (i - g * G) + 1], size = hi > lo ? hi - lo : 0;
            if (!size) { i++; continue; }
            if (c.entries && c.sum + size > limit) break;
            c.sum += size; c.entries++; i++;
            if (c.sum >= limit) break;
        }
        c.i1 = i;
        if (c.entries) chunks->push_back(c);
    }
    return DEBWT_OK;
}

struct FmSpecList {                                     // the list side of a run; null for a histogram
    u32 min_mult, max_mult;
    u64 capacity;                                       // 0: count only
    std::vector<std::pair<u64, u32>> members;
    u64 count = 0;
};

// members staged on the device to the host
int fm_spectrum_flush(debwt_fm *f, FmSpecList *ls, std::vector<u64> *hc, std::vector<u32> *hm, u64 stage) {
    u64 cnt = 0;
    HIPCHK(f, hipMemcpyAsync(&cnt, f->sp_ctr.as<u64>() + FM_SP_LIST, 8, hipMemcpyDeviceToHost, f->stream));
    int rc = fm_sync(f);
    if (rc) return rc;
    if (cnt > stage) { f->err = "spectrum: the list staging overflowed"; return DEBWT_EINTERNAL; }
    ls->count += cnt;
    if (cnt && ls->count <= ls->capacity) {
        hc->resize(cnt); hm->resize(cnt);
        HIPCHK(f, hipMemcpyAsync(hc->data(), f->sp_codes.p, (size_t)cnt * 8, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(f, hipMemcpyAsync(hm->data(), f->sp_mults.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
        for (u64 i = 0; i < cnt; i++) ls->members.emplace_back((*hc)[i], (*hm)[i]);
    }
    HIPCHK(f, hipMemsetAsync(f->sp_ctr.as<u64>() + FM_SP_LIST, 0, 8, f->stream));
    return DEBWT_OK;
}

// the walk of both calls: hist (nbins u64, host) and totals for the histogram, ls for the list
int fm_spectrum_run(debwt_fm *f, const char *what, u32 k, u32 flags, u32 nbins, uint64_t *hist, debwt_fm_spectrum_totals *totals,
                    FmSpecList *ls) {
    const auto t0 = std::chrono::steady_clock::now();
    f->sp_stats = debwt_fm_spectrum_stats{};
    debwt_fm_spectrum_stats &st = f->sp_stats;
    if (k < 1 || k > FM_SPEC_MAX_K) { f->err = std::string(what) + ": k must be 1..32"; return DEBWT_EINVAL; }
    if (flags & ~DEBWT_FM_BOTH_STRANDS) { f->err = std::string(what) + ": unknown flags"; return DEBWT_EINVAL; }
    u32 q = 0;
    int rc = fm_kmer_env_q(f, &q);
    if (rc) return rc;
    if (k < q) q = 0;
    const u64 limit = fm_env_u64("DEBWT_FM_SPECTRUM_ITEMS", FM_SPECTRUM_ITEMS);
    const u32 both = (flags & DEBWT_FM_BOTH_STRANDS) ? 1u : 0u;
    st.items_limit = limit;
    HIPCHK(f, hipSetDevice(f->device));
    FmKmerCall ev;                                             // its two events
    HIPCHK(f, hipEventCreate(&ev.e0));
    HIPCHK(f, hipEventCreate(&ev.e1));
    debwt_fm_kmer_stats kst{};
    if ((rc = fm_kmer_table(f, q, &kst))) return rc;
    st.table_q = q; st.ms_table = kst.ms_table; st.launches = kst.launches;
    std::vector<FmSpecChunk> chunks;
    if ((rc = fm_spectrum_plan(f, q, limit, &chunks, &st))) return rc;
    u64 cap = 1;
    for (const FmSpecChunk &c : chunks) cap = std::max<u64>(cap, c.sum);
    const bool stage_list = ls && ls->capacity;
    const u64 stage = stage_list ? std::max<u64>(cap, FM_SPECTRUM_STAGE) : 0;
    FM_ENSURE(f, f->sp_front, (size_t)cap * 48);
    FM_ENSURE(f, f->sp_ctr, FM_SP_NCTR * 8);
    if (hist) FM_ENSURE(f, f->sp_hist, (size_t)nbins * 8);
    if (stage_list) { FM_ENSURE(f, f->sp_codes, (size_t)stage * 8); FM_ENSURE(f, f->sp_mults, (size_t)stage * 4); }
    st.scratch_bytes = cap * 48 + FM_SP_NCTR * 8 + (hist ? (u64)nbins * 8 : 0) + stage * 12 + (q ? ((1ull << (2 * q)) + 1023) / 1024 * 16 : 0);
    HIPCHK(f, hipMemsetAsync(f->sp_ctr.p, 0, FM_SP_NCTR * 8, f->stream));
    if (hist) HIPCHK(f, hipMemsetAsync(f->sp_hist.p, 0, (size_t)nbins * 8, f->stream));
    u64 *front[2] = {f->sp_front.as<u64>(), f->sp_front.as<u64>() + 3 * cap}, *ctr = f->sp_ctr.as<u64>();
    const u64 *table = q ? f->k_table.as<u64>() : nullptr;
    std::vector<u64> hc;
    std::vector<u32> hm;
    u64 staged = 0;                                            // bound of the members on the device
    st.levels = k - q;
    (void)hipEventRecord(ev.e0, f->stream);
    for (const FmSpecChunk &c : chunks) {
        if (stage_list && staged + c.sum > stage) {
            if ((rc = fm_spectrum_flush(f, ls, &hc, &hm, stage))) return rc;
            staged = 0;
        }
        HIPCHK(f, hipMemsetAsync(ctr + FM_SP_CUR, 0, (FM_SPEC_MAX_K + 2) * 8, f->stream));
        k_fm_spectrum_start<<<grid_for(c.i1 - c.i0, 256), 256, 0, f->stream>>>(f->V, table, c.i0, c.i1, q, front[0], cap, ctr);
        u64 bound = c.entries;                                 // of the frontier of depth d
        for (u32 d = q; d < k; d++) {
            bound = std::min<u64>(bound, c.sum);
            k_fm_spectrum_expand<<<grid_for(bound, 256), 256, 0, f->stream>>>(f->V, front[(d - q) & 1], front[(d - q + 1) & 1], cap, d, ctr);
            bound = bound > c.sum / 4 ? c.sum : bound * 4;
        }
        bound = std::min<u64>(bound, c.sum);
        k_fm_spectrum_leaves<<<grid_for(bound, 256), 256, hist ? nbins * 4 : 0, f->stream>>>(
            f->V, table, q, front[(k - q) & 1], cap, k, both, nbins, hist ? f->sp_hist.as<u64>() : nullptr,
            ls ? ls->min_mult : 0, ls ? ls->max_mult : 0, stage_list ? f->sp_codes.as<u64>() : nullptr,
            stage_list ? f->sp_mults.as<u32>() : nullptr, stage, ctr);
        st.launches += 2 + (k - q);
        st.chunks++;
        staged += c.sum;
    }
    (void)hipEventRecord(ev.e1, f->stream);
    if (stage_list) { if ((rc = fm_spectrum_flush(f, ls, &hc, &hm, stage))) return rc; }
    u64 h[FM_SP_NCTR];
    HIPCHK(f, hipMemcpyAsync(h, ctr, FM_SP_NCTR * 8, hipMemcpyDeviceToHost, f->stream));
    if (hist) HIPCHK(f, hipMemcpyAsync(hist, f->sp_hist.p, (size_t)nbins * 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_kernel, ev.e0, ev.e1);
    if (h[FM_SP_CLIPPED]) { f->err = std::string(what) + ": a frontier outgrew its bound"; return DEBWT_EINTERNAL; }
    for (u32 d = 0; d <= FM_SPEC_MAX_K; d++) st.level_intervals[d] = h[FM_SP_LEVEL + d];
    for (u32 d = 0; d < k; d++) st.expanded += st.level_intervals[d];
    st.leaves = st.level_intervals[k]; st.lookups = h[FM_SP_LOOKUPS]; st.steps = st.expanded + h[FM_SP_STEPS];
    st.line_reads = h[FM_SP_READS]; st.wave_steps = h[FM_SP_WSTEPS];
    if (totals) {                                              // the bins below the last give their own share of both sums
        *totals = debwt_fm_spectrum_totals{0, h[FM_SP_OVER], h[FM_SP_OVER]};
        for (u32 c = 0; c < nbins; c++) { totals->distinct += hist[c]; if (c + 1 < nbins) totals->total += (u64)c * hist[c]; }
    }
    if (ls && !stage_list) ls->count = h[FM_SP_LIST];
    st.ms_wall = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_spectrum(debwt_fm *f, uint32_t k, uint32_t flags, uint32_t nbins, uint64_t *hist,
                                 debwt_fm_spectrum_totals *totals) {
    if (!f || !hist || !totals) return DEBWT_EINVAL;
    if (nbins < 2 || nbins > FM_SPEC_MAX_BINS) { f->err = "debwt_fm_spectrum: nbins must be 2..4096"; return DEBWT_EINVAL; }
    return fm_spectrum_run(f, "debwt_fm_spectrum", k, flags, nbins, hist, totals, nullptr);
}

extern "C" int debwt_fm_kmer_list(debwt_fm *f, uint32_t k, uint32_t flags, uint32_t min_mult, uint32_t max_mult,
                                  uint64_t *codes, uint32_t *mults, uint64_t capacity, uint64_t *count) {
    if (!f || !count || (capacity && (!codes || !mults))) return DEBWT_EINVAL;
    if (!min_mult || min_mult > max_mult) { f->err = "debwt_fm_kmer_list: min_mult must be 1..max_mult"; return DEBWT_EINVAL; }
    FmSpecList ls{min_mult, max_mult, capacity, {}, 0};
    int rc = fm_spectrum_run(f, "debwt_fm_kmer_list", k, flags, 0, nullptr, nullptr, &ls);
    if (rc) return rc;
    *count = ls.count;
    if (capacity < ls.count) {
        f->err = "debwt_fm_kmer_list: capacity below the members (count = " + std::to_string(ls.count) + ")";
        return DEBWT_ERANGE;
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::sort(ls.members.begin(), ls.members.end());           // codes are distinct: the order is that of the codes
    for (u64 i = 0; i < ls.count; i++) { codes[i] = ls.members[i].first; mults[i] = ls.members[i].second; }
    f->sp_stats.ms_wall += (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return DEBWT_OK;
}

extern "C" int debwt_fm_spectrum_threshold(const uint64_t *hist, uint32_t nbins, uint64_t total, debwt_fm_spectrum_summary *out) {
    if (!hist || !out || nbins < 2 || nbins > FM_SPEC_MAX_BINS) return DEBWT_EINVAL;
    *out = debwt_fm_spectrum_summary{0, 0, 0};
    u32 valley = 0;
    for (u32 c = 1; c + 3 <= nbins; c++)
        if (hist[c + 1] > hist[c]) { valley = c; break; }
    if (!valley) return DEBWT_OK;
    u32 peak = valley + 1;
    for (u32 c = valley + 1; c + 2 <= nbins; c++)
        if (hist[c] > hist[peak]) peak = c;
    u64 below = 0;
    for (u32 c = 1; c < valley; c++) below += (u64)c * hist[c];
    out->valley = valley; out->peak = peak;
    out->est_size = (total > below ? total - below : 0) / peak;
    return DEBWT_OK;
}

extern "C" int debwt_fm_spectrum_stats_get(const debwt_fm *f, debwt_fm_spectrum_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->sp_stats;
    return DEBWT_OK;
}

// ---- suffix array, LCP array and record array (fm_esa_kernels.h) ---------------------------------------------------------
// One build is a run of launches on the index's stream: the walk that writes the suffix array (synchronised: its chain
// check decides whether anything is kept), then scatter, PLCP, rows and the first row of the maximum without a host round
// trip.  Everything is allocated into temporaries that are released on every way out; the arrays to keep change hands
// only after the last check.

namespace {

constexpr u64 FM_ESA_CHUNK = 256;                      // text positions per lane of the PLCP kernel

void fm_esa_drop(debwt_fm *f) {
    if (!f->has_esa && !f->esa_lcp.p && !f->esa_sa.p && !f->esa_da.p && !f->rec_P.p) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (DevBuf *b : {&f->esa_lcp, &f->esa_sa, &f->esa_da, &f->rec_P}) {
        if (b->p) (void)hipFree(b->p);
        b->p = nullptr; b->cap = 0;
    }
    f->has_esa = false;
    f->esa_distinct.clear();
}

void fm_esa_keep(DevBuf &b, FmTmp &t, size_t bytes) { b.p = t.p; b.cap = bytes; t.p = nullptr; }

}  // namespace

extern "C" int debwt_fm_esa_build(debwt_fm *f, uint32_t max_lcp, uint32_t flags) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->esa_stats = debwt_fm_esa_stats{};
    debwt_fm_esa_stats &st = f->esa_stats;
    if (flags & ~(DEBWT_FM_ESA_SA | DEBWT_FM_ESA_DA)) { f->err = "debwt_fm_esa_build: unknown flags"; return DEBWT_EINVAL; }
    const u64 n = f->n, nrec = f->nrec;
    const bool keep_sa = flags & DEBWT_FM_ESA_SA, keep_da = flags & DEBWT_FM_ESA_DA;
    if (keep_da && nrec >> 32) { f->err = "debwt_fm_esa_build: the record array holds u32, the index has 2^32 records or more"; return DEBWT_EINVAL; }
    HIPCHK(f, hipSetDevice(f->device));
    fm_esa_drop(f);
    int rc;
    if (!f->has_text) {
        const auto t1 = std::chrono::steady_clock::now();
        if ((rc = debwt_fm_restore_text(f))) return rc;
        st.ms_text = (float)fm_ms_since(t1);
    } else if ((rc = fm_anchors_build(f))) return rc;
    const u64 cap = max_lcp ? max_lcp : 0xFFFFFFFFull;
    const u64 chunk = fm_env_u64("DEBWT_FM_ESA_CHUNK", FM_ESA_CHUNK), nchunks = (n + chunk - 1) / chunk;
    st.chunk_len = chunk; st.chunks = nchunks;
    const size_t sbw = (size_t)((n + 63) >> 6) + 2, small_bytes = (size_t)(FM_ESA_NCTR + FM_ESA_NDIFF) * 8;
    const u64 rkw = (n + 63) >> 6, rkc = (rkw + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;   // the rank over the bitmap
    FmTmp sa, phi, plcp, lcp, da, sepbits, seps, wpre, csum, small;
    HIPCHK(f, hipMalloc(&sa.p, (size_t)n * 8));
    HIPCHK(f, hipMalloc(&phi.p, (size_t)n * 8));
    HIPCHK(f, hipMalloc(&plcp.p, (size_t)n * 4));
    HIPCHK(f, hipMalloc(&lcp.p, (size_t)n * 4));
    if (keep_da) HIPCHK(f, hipMalloc(&da.p, (size_t)n * 4));
    HIPCHK(f, hipMalloc(&sepbits.p, sbw * 8));
    HIPCHK(f, hipMalloc(&seps.p, (size_t)nrec * 8));
    HIPCHK(f, hipMalloc(&wpre.p, (size_t)rkw * 4));
    HIPCHK(f, hipMalloc(&csum.p, (size_t)(rkc + 1) * 8));
    HIPCHK(f, hipMalloc(&small.p, small_bytes));
    st.build_bytes = n * 24 + (keep_da ? n * 4 : 0) + sbw * 8 + nrec * 8 + rkw * 4 + (rkc + 1) * 8 + small_bytes;
    u64 *d_sa = reinterpret_cast<u64 *>(sa.p), *d_phi = reinterpret_cast<u64 *>(phi.p), *d_bits = reinterpret_cast<u64 *>(sepbits.p);
    u64 *d_seps = reinterpret_cast<u64 *>(seps.p), *d_csum = reinterpret_cast<u64 *>(csum.p), *ctr = reinterpret_cast<u64 *>(small.p);
    u32 *d_plcp = reinterpret_cast<u32 *>(plcp.p), *d_lcp = reinterpret_cast<u32 *>(lcp.p), *d_da = reinterpret_cast<u32 *>(da.p);

    // the suffix array: one walk over every anchor gap; the extract statistics stay those of the last extract or restore
    FM_ENSURE(f, f->e_ctr, 64);
    const debwt_fm_extract_stats e_keep = f->e_stats;
    f->e_stats = debwt_fm_extract_stats{};
    u64 h[8];
    rc = fm_extract_walk(f, FmExSa{d_sa}, f->na - 1, false, h);
    st.walk_items = f->na - 1; st.walk_steps = f->e_stats.steps; st.walk_wave_steps = f->e_stats.wave_steps;
    st.ms_walk = f->e_stats.ms_kernel;
    f->e_stats = e_keep;
    if (rc) return rc;
    if (h[FM_EX_W_CHAIN] || h[FM_EX_W_BAD] || h[FM_EX_W_STEPS] != n - 1) {
        f->err = "debwt_fm_esa_build: the samples are not those of the rows (" + std::to_string(h[FM_EX_W_CHAIN]) +
                 " walks missed the row of their lower anchor or the '$' row at the text's start, " +
                 std::to_string(h[FM_EX_W_BAD]) + " were refused, " + std::to_string(h[FM_EX_W_STEPS]) + " of " +
                 std::to_string(n - 1) + " steps)";
        return DEBWT_EINVAL;
    }

    std::vector<u64> hs(nrec);                                 // the separator positions
    for (u64 r = 0; r < nrec; r++) hs[r] = (r + 1 < nrec ? f->rec_starts[r + 1] : n) - 1;
    HIPCHK(f, hipMemcpyAsync(d_seps, hs.data(), (size_t)nrec * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(d_bits, 0, sbw * 8, f->stream));
    HIPCHK(f, hipMemsetAsync(ctr, 0, small_bytes, f->stream));
    HIPCHK(f, hipMemsetAsync(ctr + FM_ESA_C_MAXROW, 0xFF, 8, f->stream));
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < 4; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < 4; i++) HIPCHK(f, hipEventCreate(&ev[i]));
    k_set_sepbits<<<grid_for(nrec, 256), 256, 0, f->stream>>>(d_seps, nrec, d_bits);
    k_fm_anc_count<<<(u32)rkc, FM_EX_CHUNK_WORDS, 0, f->stream>>>(d_bits, rkw, reinterpret_cast<u32 *>(wpre.p), d_csum);
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(d_csum, rkc, d_csum + rkc);
    (void)hipEventRecord(ev[0], f->stream);
    k_fm_esa_phi<<<grid_for(n, 256), 256, 0, f->stream>>>(d_sa, n, d_phi);
    (void)hipEventRecord(ev[1], f->stream);
    k_fm_esa_plcp<<<grid_for(nchunks, 256), 256, 0, f->stream>>>(f->text.as<u64>(), d_bits, d_phi, n, chunk, nchunks, cap, d_plcp, ctr);
    (void)hipEventRecord(ev[2], f->stream);
    // few workgroups with many rows each: the per-wave sums and the flush of the LDS array are atomics on shared addresses
    const u32 row_blocks = (u32)std::min<u64>(grid_for(n, 256), std::max<u64>(4096, (n >> 30) + 1));
    k_fm_esa_rows<<<row_blocks, 256, 0, f->stream>>>(d_sa, d_plcp, d_bits, reinterpret_cast<const u32 *>(wpre.p), d_csum, d_seps,
                                                     nrec, n, (u32)cap, max_lcp ? 1u : 0u, d_lcp, keep_da ? d_da : nullptr, ctr,
                                                     ctr + FM_ESA_NCTR);
    k_fm_esa_maxrow<<<grid_for(n, 256), 256, 0, f->stream>>>(d_lcp, n, ctr);
    (void)hipEventRecord(ev[3], f->stream);
    std::vector<u64> hc(FM_ESA_NCTR + FM_ESA_NDIFF);
    HIPCHK(f, hipMemcpyAsync(hc.data(), ctr, small_bytes, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_scatter, ev[0], ev[1]);
    (void)hipEventElapsedTime(&st.ms_plcp, ev[1], ev[2]);
    (void)hipEventElapsedTime(&st.ms_rows, ev[2], ev[3]);
    if (hc[FM_ESA_C_BADPHI] || hc[FM_ESA_C_MAXROW] >= n) {
        f->err = "debwt_fm_esa_build: the suffix array is no permutation of the text positions";
        return DEBWT_EINTERNAL;
    }
    st.symbols_compared = hc[FM_ESA_C_SYMBOLS]; st.plcp_wave_steps = hc[FM_ESA_C_WAVE];
    debwt_fm_esa_summary &sm = f->esa_sum;
    sm = debwt_fm_esa_summary{n, hc[FM_ESA_C_MAX], hc[FM_ESA_C_MAXROW], hc[FM_ESA_C_SUM], hc[FM_ESA_C_CAPPED], 0, 0, cap};
    u64 pos[2] = {0, 0};
    const u64 r0 = sm.max_row ? sm.max_row - 1 : 0;
    HIPCHK(f, hipMemcpyAsync(pos, d_sa + r0, sm.max_row ? 16 : 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    sm.pos_prev = pos[0]; sm.pos = sm.max_row ? pos[1] : pos[0];
    f->esa_distinct.assign(FM_ESA_KMAX, 0);                    // distinct[k - 1] = the sum of diff[1 .. k]
    u64 run = 0;
    for (u32 k = 1; k <= FM_ESA_KMAX; k++) { run += hc[FM_ESA_NCTR + k]; f->esa_distinct[k - 1] = run; }
    fm_esa_keep(f->esa_lcp, lcp, (size_t)n * 4);
    if (keep_sa) fm_esa_keep(f->esa_sa, sa, (size_t)n * 8);
    if (keep_da) fm_esa_keep(f->esa_da, da, (size_t)n * 4);
    f->has_esa = true;
    st.kept_bytes = f->esa_lcp.cap + f->esa_sa.cap + f->esa_da.cap;
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_esa_fetch(debwt_fm *f, int which, uint64_t row_lo, uint64_t count, void *dst) {
    if (!f) return DEBWT_EINVAL;
    if (which != DEBWT_FM_ESA_LCP_ARRAY && which != DEBWT_FM_ESA_SA_ARRAY && which != DEBWT_FM_ESA_DA_ARRAY) {
        f->err = "debwt_fm_esa_fetch: which must name the LCP, SA or DA array"; return DEBWT_EINVAL;
    }
    const DevBuf &b = which == DEBWT_FM_ESA_LCP_ARRAY ? f->esa_lcp : which == DEBWT_FM_ESA_SA_ARRAY ? f->esa_sa : f->esa_da;
    if (!f->has_esa || !b.p) { f->err = "debwt_fm_esa_fetch: no build holds this array (debwt_fm_esa_build and its flags)"; return DEBWT_ESTATE; }
    if (row_lo > f->n || count > f->n - row_lo) { f->err = "debwt_fm_esa_fetch: row_lo + count exceeds n"; return DEBWT_EINVAL; }
    if (!count) return DEBWT_OK;
    if (!dst) return DEBWT_EINVAL;
    const size_t w = which == DEBWT_FM_ESA_SA_ARRAY ? 8 : 4;
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipMemcpyAsync(dst, b.as<u8>() + (size_t)row_lo * w, (size_t)count * w, hipMemcpyDeviceToHost, f->stream));
    return fm_sync(f);
}

extern "C" int debwt_fm_esa_summary_get(const debwt_fm *f, debwt_fm_esa_summary *out) {
    if (!f || !out) return DEBWT_EINVAL;
    if (!f->has_esa) return DEBWT_ESTATE;
    *out = f->esa_sum;
    return DEBWT_OK;
}

extern "C" int debwt_fm_esa_profile(debwt_fm *f, uint32_t kmax, uint64_t *distinct) {
    if (!f || !distinct) return DEBWT_EINVAL;
    if (!f->has_esa) { f->err = "debwt_fm_esa_profile: no build (debwt_fm_esa_build)"; return DEBWT_ESTATE; }
    if (!kmax || kmax > FM_ESA_KMAX || kmax > f->esa_sum.cap) {
        f->err = "debwt_fm_esa_profile: kmax must be 1..4096 and at most the cap of the build"; return DEBWT_EINVAL;
    }
    memcpy(distinct, f->esa_distinct.data(), (size_t)kmax * 8);
    return DEBWT_OK;
}

extern "C" int debwt_fm_esa_release(debwt_fm *f) {
    if (!f) return DEBWT_EINVAL;
    fm_esa_drop(f);
    return DEBWT_OK;
}

extern "C" int debwt_fm_esa_stats_get(const debwt_fm *f, debwt_fm_esa_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->esa_stats;
    return DEBWT_OK;
}

// ---- maximal and supermaximal repeats (fm_repeat_kernels.h) ------------------------------------------------------------
// One call is a run of launches on the index's stream: the levels of the hierarchy, the search, and for a call that takes
// the list the rank over the masks of the reported rows and the write.  Everything is allocated into temporaries that are
// released on every way out; the kept arrays are only read.

static_assert(sizeof(debwt_fm_repeat) == 64, "a record of debwt_fm_repeats is 64 bytes");

// filter: null for debwt_fm_repeats (who names the call in messages); records: the records of every listed interval, or null
static int fm_repeats_run(debwt_fm *f, const std::string &who, const debwt_fm_repeat_opts *opts, const debwt_fm_record_filter *filter,
                          debwt_fm_repeat *out, uint32_t *records, uint64_t capacity, uint64_t *count) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!opts || !count) { f->err = who + ": opts and count must not be NULL"; return DEBWT_EINVAL; }
    if (!opts->min_len || opts->min_occ < 2 || (opts->max_occ && opts->max_occ < opts->min_occ)) {
        f->err = who + ": min_len must be at least 1, min_occ at least 2 and max_occ 0 or at least min_occ";
        return DEBWT_EINVAL;
    }
    if (opts->kind > DEBWT_FM_REPEAT_INTERVALS) { f->err = who + ": unknown kind"; return DEBWT_EINVAL; }
    if (capacity && !out) { f->err = who + ": out is NULL with capacity > 0"; return DEBWT_EINVAL; }
    if (!f->has_esa || !f->esa_lcp.p) { f->err = who + ": no build holds the LCP array (debwt_fm_esa_build)"; return DEBWT_ESTATE; }
    if (filter && !f->rec_P.p) { f->err = who + ": no records build (debwt_fm_records_build)"; return DEBWT_ESTATE; }
    const u64 F = fm_env_u64("DEBWT_FM_REPEAT_FANOUT", 64);
    if (F < 2 || F > 64 || (F & (F - 1))) { f->err = who + ": DEBWT_FM_REPEAT_FANOUT must be a power of two in 2..64"; return DEBWT_EINVAL; }
    u32 sh = 0;
    while ((1ull << sh) < F) sh++;
    f->rp_stats = debwt_fm_repeat_stats{};
    debwt_fm_repeat_stats &st = f->rp_stats;
    const u64 n = f->n;
    HIPCHK(f, hipSetDevice(f->device));

    // the level table: n_t, and where level t begins in the node buffer
    std::vector<u64> lev{n, 0};
    u64 nodes = 0;
    for (u64 m = n; m > 1;) { m = (m + F - 1) >> sh; lev.push_back(m); lev.push_back(nodes); nodes += m; }
    const u32 levels = (u32)(lev.size() / 2 - 1);
    if (levels > FM_REP_MAXLEV) { f->err = who + ": more levels than the kernels hold"; return DEBWT_EINTERNAL; }
    const bool list = capacity != 0;
    const u64 nw = (n + 63) >> 6, rkc = (nw + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;
    const u32 blocks = (u32)std::min<u64>(grid_for(n, 256), 4096);
    const size_t small_bytes = (size_t)(FM_REP_NCTR + 2 * (FM_REP_MAXLEV + 1)) * 8, best_bytes = (size_t)blocks * 16;
    FmTmp node, small, best, lo, hi, masks, wpre, csum, dout, drec;
    HIPCHK(f, hipMalloc(&node.p, (size_t)std::max<u64>(nodes, 1) * 8));
    HIPCHK(f, hipMalloc(&small.p, small_bytes));
    HIPCHK(f, hipMalloc(&best.p, best_bytes));
    st.rows = n; st.levels = levels; st.fanout = F; st.tree_bytes = nodes * 8;
    st.scratch_bytes = st.tree_bytes + small_bytes + best_bytes;
    if (list) {
        HIPCHK(f, hipMalloc(&lo.p, (size_t)n * 8));
        HIPCHK(f, hipMalloc(&hi.p, (size_t)n * 8));
        HIPCHK(f, hipMalloc(&masks.p, (size_t)nw * 24));
        HIPCHK(f, hipMalloc(&wpre.p, (size_t)nw * 4));
        HIPCHK(f, hipMalloc(&csum.p, (size_t)(rkc + 1) * 8));
        st.scratch_bytes += n * 16 + nw * 28 + (rkc + 1) * 8;
    }
    u64 *ctr = reinterpret_cast<u64 *>(small.p), *d_lev = ctr + FM_REP_NCTR, *d_best = reinterpret_cast<u64 *>(best.p);
    uint2 *d_node = reinterpret_cast<uint2 *>(node.p);
    const u32 *d_lcp = f->esa_lcp.as<u32>();
    u64 *d_masks = reinterpret_cast<u64 *>(masks.p), *d_csum = reinterpret_cast<u64 *>(csum.p);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < 4; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < 4; i++) HIPCHK(f, hipEventCreate(&ev[i]));
    HIPCHK(f, hipMemsetAsync(ctr, 0, FM_REP_NCTR * 8, f->stream));
    HIPCHK(f, hipMemcpyAsync(d_lev, lev.data(), lev.size() * 8, hipMemcpyHostToDevice, f->stream));
    (void)hipEventRecord(ev[0], f->stream);
    for (u32 t = 0; t < levels; t++) {
        const u64 nin = lev[2 * t], nout = lev[2 * t + 2];
        const u32 g = (u32)std::min<u64>(grid_for(nin, 256), 1u << 20);
        if (t == 0) k_fm_rep_level<true><<<g, 256, 0, f->stream>>>(d_lcp, nullptr, nin, sh, d_node + lev[3], nout);
        else k_fm_rep_level<false><<<g, 256, 0, f->stream>>>(nullptr, d_node + lev[2 * t + 1], nin, sh, d_node + lev[2 * t + 3], nout);
    }
    (void)hipEventRecord(ev[1], f->stream);
    const u32 cap = f->esa_sum.cap < 0xFFFFFFFFull ? (u32)f->esa_sum.cap : 0u;
    const FmRepTree T{d_lcp, d_node, d_lev, levels, sh};
    const FmRepOpts O{opts->min_len, opts->kind, cap, opts->min_occ, opts->max_occ};
    u64 *const d_lo = reinterpret_cast<u64 *>(lo.p), *const d_hi = reinterpret_cast<u64 *>(hi.p);
    u64 *const m0 = list ? d_masks : nullptr, *const m1 = list ? d_masks + nw : nullptr, *const m2 = list ? d_masks + 2 * nw : nullptr;
    if (filter)
        k_fm_rep_search<true><<<blocks, 256, 0, f->stream>>>(f->V, T, O, d_lo, d_hi, m0, m1, m2, ctr, d_best, f->rec_P.as<u64>(),
                                                             FmRecFilter{filter->min_records, filter->max_records, filter->flags});
    else
        k_fm_rep_search<false><<<blocks, 256, 0, f->stream>>>(f->V, T, O, d_lo, d_hi, m0, m1, m2, ctr, d_best, nullptr, FmRecFilter{});
    (void)hipEventRecord(ev[2], f->stream);
    u64 hc[FM_REP_NCTR];
    std::vector<u64> hb((size_t)blocks * 2);
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(hb.data(), d_best, best_bytes, hipMemcpyDeviceToHost, f->stream));
    int rc;
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_tree, ev[0], ev[1]);
    (void)hipEventElapsedTime(&st.ms_search, ev[1], ev[2]);
    st.searched = hc[FM_REP_C_SEARCHED]; st.representatives = hc[FM_REP_C_REPS]; st.capped_intervals = hc[FM_REP_C_CAPPED];
    st.intervals = st.representatives - st.capped_intervals;
    st.maximal = hc[FM_REP_C_MAXIMAL]; st.supermaximal = hc[FM_REP_C_SUPER]; st.reported = hc[FM_REP_C_REPORTED];
    st.search_steps = hc[FM_REP_C_STEPS]; st.wave_steps = hc[FM_REP_C_WAVE]; st.rank_lines = hc[FM_REP_C_LINES];
    for (u32 b = 0; b < blocks; b++)
        if (hb[2 * b] > st.longest_len || (hb[2 * b] && hb[2 * b] == st.longest_len && hb[2 * b + 1] < st.longest_row_lo)) {
            st.longest_len = hb[2 * b]; st.longest_row_lo = hb[2 * b + 1];
        }
    *count = st.reported;
    if (capacity < st.reported) {
        st.ms_wall = (float)fm_ms_since(t0);
        f->err = who + ": capacity below the repeats (count = " + std::to_string(st.reported) + ")";
        return DEBWT_ERANGE;
    }
    if (st.reported) {
        HIPCHK(f, hipMalloc(&dout.p, (size_t)st.reported * sizeof(debwt_fm_repeat)));
        st.scratch_bytes += st.reported * sizeof(debwt_fm_repeat);
        if (records) {
            HIPCHK(f, hipMalloc(&drec.p, (size_t)st.reported * 4));
            st.scratch_bytes += st.reported * 4;
        }
        k_fm_anc_count<<<(u32)rkc, FM_EX_CHUNK_WORDS, 0, f->stream>>>(d_masks, nw, reinterpret_cast<u32 *>(wpre.p), d_csum);
        k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(d_csum, rkc, d_csum + rkc);
        k_fm_rep_write<<<(u32)std::min<u64>(grid_for(n, 256), 1u << 20), 256, 0, f->stream>>>(
            f->V, d_lcp, n, reinterpret_cast<const u64 *>(lo.p), reinterpret_cast<const u64 *>(hi.p), d_masks, d_masks + nw,
            d_masks + 2 * nw, reinterpret_cast<const u32 *>(wpre.p), d_csum, reinterpret_cast<debwt_fm_repeat *>(dout.p), st.reported,
            records ? f->rec_P.as<u64>() : nullptr, reinterpret_cast<u32 *>(drec.p));
        (void)hipEventRecord(ev[3], f->stream);
        u64 total = 0;
        HIPCHK(f, hipMemcpyAsync(&total, d_csum + rkc, 8, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(f, hipMemcpyAsync(out, dout.p, (size_t)st.reported * sizeof(debwt_fm_repeat), hipMemcpyDeviceToHost, f->stream));
        if (records) HIPCHK(f, hipMemcpyAsync(records, drec.p, (size_t)st.reported * 4, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
        (void)hipEventElapsedTime(&st.ms_write, ev[2], ev[3]);
        st.rank_lines += 8 * st.reported;
        if (total != st.reported) { f->err = who + ": the masks and the count of the reported rows differ"; return DEBWT_EINTERNAL; }
    }
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_repeats(debwt_fm *f, const debwt_fm_repeat_opts *opts, debwt_fm_repeat *out, uint64_t capacity,
                                uint64_t *count) {
    if (!f) return DEBWT_EINVAL;
    return fm_repeats_run(f, "debwt_fm_repeats", opts, nullptr, out, nullptr, capacity, count);
}

extern "C" int debwt_fm_repeat_stats_get(const debwt_fm *f, debwt_fm_repeat_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->rp_stats;
    return DEBWT_OK;
}

// ---- distinct records per LCP interval (fm_record_kernels.h) -----------------------------------------------------------
// The build is one run of launches on the index's stream: keys, the stable passes over the record bits, the hierarchy of
// the repeats section, one range minimum per pair, the prefix sum.  Everything is allocated into temporaries that are
// released on every way out; the prefix changes hands only after the last check, so a failed build leaves an earlier
// prefix in place.

namespace {

u32 fm_bits_of(u64 v) { u32 b = 0; while (b < 64 && (v >> b)) b++; return b; }    // the bits of v; 0 for v = 0

template <typename DT>
void fm_records_launch(debwt_fm *f, const FmRepTree &T, const u64 *keys, u32 rb, void *dup, u64 *ctr, u64 *tsum, u64 ntiles, u64 *P,
                       hipEvent_t after_pairs) {
    const u64 n = f->n;
    DT *d_dup = reinterpret_cast<DT *>(dup);
    k_fm_rec_pairs<DT><<<(u32)std::min<u64>(grid_for(n, 256), 4096), 256, 0, f->stream>>>(T, keys, rb, d_dup, ctr);
    (void)hipEventRecord(after_pairs, f->stream);
    k_fm_rec_tile_sums<DT><<<(u32)ntiles, FM_REC_TILE, 0, f->stream>>>(d_dup, n, tsum);
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(tsum, ntiles, tsum + ntiles);
    k_fm_rec_scan<DT><<<(u32)ntiles, FM_REC_TILE, 0, f->stream>>>(d_dup, n, tsum, P);
}

}  // namespace

extern "C" int debwt_fm_records_build(debwt_fm *f) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    if (!f->has_esa || !f->esa_lcp.p || !f->esa_da.p) {
        f->err = "debwt_fm_records_build: no build holds the record array (debwt_fm_esa_build with DEBWT_FM_ESA_DA)";
        return DEBWT_ESTATE;
    }
    const u64 F = fm_env_u64("DEBWT_FM_REPEAT_FANOUT", 64);
    if (F < 2 || F > 64 || (F & (F - 1))) { f->err = "debwt_fm_records_build: DEBWT_FM_REPEAT_FANOUT must be a power of two in 2..64"; return DEBWT_EINVAL; }
    u32 sh = 0;
    while ((1ull << sh) < F) sh++;
    const u64 n = f->n, nrec = f->nrec;
    const u32 rb = fm_bits_of(n - 1), db = fm_bits_of(nrec - 1);
    if (rb + db > 64) { f->err = "debwt_fm_records_build: record and row do not fit one 64-bit key"; return DEBWT_EINVAL; }
    if ((n + FM_REC_TILE - 1) / FM_REC_TILE > 0x7FFFFFFFull) { f->err = "debwt_fm_records_build: more rows than the scan's grid holds"; return DEBWT_EINVAL; }
    debwt_fm_records_stats st{};
    HIPCHK(f, hipSetDevice(f->device));

    std::vector<u64> lev{n, 0};                                // the level table of debwt_fm_repeats
    u64 nodes = 0;
    for (u64 m = n; m > 1;) { m = (m + F - 1) >> sh; lev.push_back(m); lev.push_back(nodes); nodes += m; }
    const u32 levels = (u32)(lev.size() / 2 - 1);
    if (levels > FM_REP_MAXLEV) { f->err = "debwt_fm_records_build: more levels than the kernels hold"; return DEBWT_EINTERNAL; }
    const bool wide = n >> 32;                                 // dup as u64
    const u64 ntiles = (n + FM_REC_TILE - 1) / FM_REC_TILE;
    const size_t small_bytes = (size_t)(FM_REC_NCTR + 2 * (FM_REP_MAXLEV + 1)) * 8, ws_bytes = radix_workspace_bytes(n),
                 dup_bytes = (size_t)n * (wide ? 8 : 4), tsum_bytes = (size_t)(ntiles + 1) * 8;
    FmTmp ka, kb, rws, node, small, dup, tsum, P;
    HIPCHK(f, hipMalloc(&ka.p, (size_t)n * 8));
    HIPCHK(f, hipMalloc(&kb.p, (size_t)n * 8));
    HIPCHK(f, hipMalloc(&rws.p, ws_bytes));
    HIPCHK(f, hipMalloc(&node.p, (size_t)std::max<u64>(nodes, 1) * 8));
    HIPCHK(f, hipMalloc(&small.p, small_bytes));
    HIPCHK(f, hipMalloc(&dup.p, dup_bytes));
    HIPCHK(f, hipMalloc(&tsum.p, tsum_bytes));
    HIPCHK(f, hipMalloc(&P.p, (size_t)n * 8));
    st.rows = n; st.levels = levels; st.fanout = F; st.sort_passes = (db + 7) / 8;
    st.kept_bytes = n * 8;
    st.build_bytes = n * 16 + ws_bytes + std::max<u64>(nodes, 1) * 8 + small_bytes + dup_bytes + tsum_bytes + st.kept_bytes;
    u64 *ctr = reinterpret_cast<u64 *>(small.p), *d_lev = ctr + FM_REC_NCTR;
    uint2 *d_node = reinterpret_cast<uint2 *>(node.p);
    const u32 *d_lcp = f->esa_lcp.as<u32>();
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < 5; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < 5; i++) HIPCHK(f, hipEventCreate(&ev[i]));
    HIPCHK(f, hipMemsetAsync(ctr, 0, FM_REC_NCTR * 8, f->stream));
    HIPCHK(f, hipMemsetAsync(dup.p, 0, dup_bytes, f->stream));
    HIPCHK(f, hipMemcpyAsync(d_lev, lev.data(), lev.size() * 8, hipMemcpyHostToDevice, f->stream));
    (void)hipEventRecord(ev[0], f->stream);
    k_fm_rec_keys<<<(u32)std::min<u64>(grid_for(n, 256), 1u << 20), 256, 0, f->stream>>>(f->esa_da.as<u32>(), n, rb,
                                                                                         reinterpret_cast<u64 *>(ka.p));
    RadixWorkspace ws{};
    ws.counts = reinterpret_cast<u32 *>(rws.p);                // chunk histograms only: no pair counts, no hybrid lists
    hipError_t e = hipSuccess;
    const u64 *sorted = radix_sort_bits(f->stream, reinterpret_cast<u64 *>(ka.p), reinterpret_cast<u64 *>(kb.p), n, (int)rb,
                                        (int)(rb + db), ws, &e);
    if (e != hipSuccess) { f->err = std::string("debwt_fm_records_build: the key sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
    (void)hipEventRecord(ev[1], f->stream);
    for (u32 t = 0; t < levels; t++) {
        const u64 nin = lev[2 * t], nout = lev[2 * t + 2];
        const u32 g = (u32)std::min<u64>(grid_for(nin, 256), 1u << 20);
        if (t == 0) k_fm_rep_level<true><<<g, 256, 0, f->stream>>>(d_lcp, nullptr, nin, sh, d_node + lev[3], nout);
        else k_fm_rep_level<false><<<g, 256, 0, f->stream>>>(nullptr, d_node + lev[2 * t + 1], nin, sh, d_node + lev[2 * t + 3], nout);
    }
    (void)hipEventRecord(ev[2], f->stream);
    const FmRepTree T{d_lcp, d_node, d_lev, levels, sh};
    if (wide) fm_records_launch<u64>(f, T, sorted, rb, dup.p, ctr, reinterpret_cast<u64 *>(tsum.p), ntiles, reinterpret_cast<u64 *>(P.p), ev[3]);
    else fm_records_launch<u32>(f, T, sorted, rb, dup.p, ctr, reinterpret_cast<u64 *>(tsum.p), ntiles, reinterpret_cast<u64 *>(P.p), ev[3]);
    (void)hipEventRecord(ev[4], f->stream);
    u64 hc[FM_REC_NCTR], total = 0;
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(&total, reinterpret_cast<u64 *>(tsum.p) + ntiles, 8, hipMemcpyDeviceToHost, f->stream));
    int rc;
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_sort, ev[0], ev[1]);
    (void)hipEventElapsedTime(&st.ms_tree, ev[1], ev[2]);
    (void)hipEventElapsedTime(&st.ms_pairs, ev[2], ev[3]);
    (void)hipEventElapsedTime(&st.ms_scan, ev[3], ev[4]);
    st.pairs = hc[FM_REC_C_PAIRS]; st.records_present = n - st.pairs;
    st.rmq_steps = hc[FM_REC_C_STEPS]; st.wave_steps = hc[FM_REC_C_WAVE];
    if (hc[FM_REC_C_LOST] || total != st.pairs || st.pairs >= n) {
        f->err = "debwt_fm_records_build: the pairs and the sum of dup differ (" + std::to_string(st.pairs) + " pairs, " +
                 std::to_string(total) + " counted, " + std::to_string(hc[FM_REC_C_LOST]) + " without a minimum)";
        return DEBWT_EINTERNAL;
    }
    if (f->rec_P.p) (void)hipFree(f->rec_P.p);                 // a second build replaces the first
    fm_esa_keep(f->rec_P, P, (size_t)n * 8);
    st.ms_wall = (float)fm_ms_since(t0);
    f->rc_stats = st;
    return DEBWT_OK;
}

extern "C" int debwt_fm_records_fetch(debwt_fm *f, uint64_t row_lo, uint64_t count, uint64_t *P) {
    if (!f) return DEBWT_EINVAL;
    if (!f->has_esa || !f->rec_P.p) { f->err = "debwt_fm_records_fetch: no records build (debwt_fm_records_build)"; return DEBWT_ESTATE; }
    if (row_lo > f->n || count > f->n - row_lo) { f->err = "debwt_fm_records_fetch: row_lo + count exceeds n"; return DEBWT_EINVAL; }
    if (!count) return DEBWT_OK;
    if (!P) return DEBWT_EINVAL;
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipMemcpyAsync(P, f->rec_P.as<u64>() + row_lo, (size_t)count * 8, hipMemcpyDeviceToHost, f->stream));
    return fm_sync(f);
}

extern "C" int debwt_fm_record_counts(debwt_fm *f, const uint64_t *ranges, uint64_t nranges, uint64_t *records) {
    if (!f) return DEBWT_EINVAL;
    if (!f->has_esa || !f->rec_P.p) { f->err = "debwt_fm_record_counts: no records build (debwt_fm_records_build)"; return DEBWT_ESTATE; }
    if (!nranges) return DEBWT_OK;
    if (!ranges || !records) { f->err = "debwt_fm_record_counts: ranges and records must not be NULL"; return DEBWT_EINVAL; }
    for (u64 k = 0; k < nranges; k++)
        if (ranges[2 * k + 1] > f->n || ranges[2 * k] > ranges[2 * k + 1]) {
            f->err = "debwt_fm_record_counts: range " + std::to_string(k) + " has hi > n or lo > hi"; return DEBWT_EINVAL;
        }
    HIPCHK(f, hipSetDevice(f->device));
    FmTmp dr, dout;
    HIPCHK(f, hipMalloc(&dr.p, (size_t)nranges * 16));
    HIPCHK(f, hipMalloc(&dout.p, (size_t)nranges * 8));
    HIPCHK(f, hipMemcpyAsync(dr.p, ranges, (size_t)nranges * 16, hipMemcpyHostToDevice, f->stream));
    k_fm_rec_gather<<<(u32)std::min<u64>(grid_for(nranges, 256), 1u << 20), 256, 0, f->stream>>>(
        f->rec_P.as<u64>(), f->n, reinterpret_cast<const u64 *>(dr.p), nranges, reinterpret_cast<u64 *>(dout.p));
    HIPCHK(f, hipMemcpyAsync(records, dout.p, (size_t)nranges * 8, hipMemcpyDeviceToHost, f->stream));
    return fm_sync(f);
}

extern "C" int debwt_fm_repeats_records(debwt_fm *f, const debwt_fm_repeat_opts *opts, const debwt_fm_record_filter *filter,
                                        debwt_fm_repeat *out, uint32_t *records, uint64_t capacity, uint64_t *count) {
    if (!f) return DEBWT_EINVAL;
    if (!filter) { f->err = "debwt_fm_repeats_records: filter must not be NULL"; return DEBWT_EINVAL; }
    if (!filter->min_records || (filter->max_records && filter->max_records < filter->min_records) ||
        (filter->flags & ~DEBWT_FM_RECORDS_UNIQUE) || filter->reserved) {
        f->err = "debwt_fm_repeats_records: min_records must be at least 1, max_records 0 or at least min_records, flags known and reserved 0";
        return DEBWT_EINVAL;
    }
    return fm_repeats_run(f, "debwt_fm_repeats_records", opts, filter, out, records, capacity, count);
}

extern "C" int debwt_fm_records_stats_get(const debwt_fm *f, debwt_fm_records_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->rc_stats;
    return DEBWT_OK;
}

// ---- compacted de Bruijn graph (fm_cdbg_kernels.h) ----------------------------------------------------------------------
// One call is a run of launches on the index's stream: the three bitmaps over the rows and their ranks, degrees and links
// per piece, the ranking rounds (the host reads four counters after each: the list's length, the nodes finished, the
// cycles found), the first nodes, and for a call that takes the graph the unitig records, the strings and the sorted edge
// keys.  Everything is allocated into temporaries that are released on every way out; the kept arrays are only read.

static_assert(sizeof(debwt_fm_unitig) == 32, "a record of debwt_fm_cdbg is 32 bytes");
static_assert(sizeof(debwt_fm_cdbg_edge) == 8, "an edge of debwt_fm_cdbg is 8 bytes");

extern "C" int debwt_fm_cdbg(debwt_fm *f, uint32_t k, uint32_t flags, debwt_fm_unitig *unitigs, uint64_t unitig_capacity,
                             uint8_t *seq, uint64_t seq_capacity, debwt_fm_cdbg_edge *edges, uint64_t edge_capacity,
                             debwt_fm_cdbg_sizes *sizes) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    if (!sizes) { f->err = "debwt_fm_cdbg: sizes must not be NULL"; return DEBWT_EINVAL; }
    if (!k) { f->err = "debwt_fm_cdbg: k must be at least 1"; return DEBWT_EINVAL; }
    if (flags) { f->err = "debwt_fm_cdbg: unknown flags"; return DEBWT_EINVAL; }
    if ((unitig_capacity && !unitigs) || (seq_capacity && !seq) || (edge_capacity && !edges)) {
        f->err = "debwt_fm_cdbg: an array is NULL with capacity > 0"; return DEBWT_EINVAL;
    }
    if (!f->has_esa || !f->esa_lcp.p || !f->esa_sa.p || !f->esa_da.p) {
        f->err = "debwt_fm_cdbg: no build holds lcp, sa and da (debwt_fm_esa_build with DEBWT_FM_ESA_SA | DEBWT_FM_ESA_DA)";
        return DEBWT_ESTATE;
    }
    if ((u64)k + 1 > f->esa_sum.cap) {
        f->err = "debwt_fm_cdbg: k + 1 is above the cap of the build (" + std::to_string(f->esa_sum.cap) + ")"; return DEBWT_EINVAL;
    }
    if (f->n >> 32) { f->err = "debwt_fm_cdbg: the index has 2^32 rows or more"; return DEBWT_EINVAL; }
    f->dbg_stats = debwt_fm_cdbg_stats{};
    debwt_fm_cdbg_stats &st = f->dbg_stats;
    HIPCHK(f, hipSetDevice(f->device));
    int rc;
    if (!f->has_text && (rc = debwt_fm_restore_text(f))) return rc;
    const u64 n = f->n, nrec = f->nrec;
    auto grid = [](u64 m) { return (u32)std::min<u64>(std::max<u64>(grid_for(m, 256), 1), 1u << 20); };
    // few workgroups with many items each where a kernel ends in atomics on shared counters or stages a list in LDS
    auto few = [](u64 m, u64 per) { return (u32)std::min<u64>(std::max<u64>((m + per - 1) / per, 1), 4096); };
    auto take = [&st](FmTmp &t, size_t bytes) { st.scratch_bytes += bytes; return hipMalloc(&t.p, std::max<size_t>(bytes, 8)); };

    // rows: three bitmaps of one word more than the rows need, ranks over the start and the out bits
    const u64 nbw = (n >> 6) + 1, rkc = (nbw + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;
    FmTmp bits, wpre, csum, seps, small;
    HIPCHK(f, take(bits, (size_t)nbw * 24));
    HIPCHK(f, take(wpre, (size_t)nbw * 8));
    HIPCHK(f, take(csum, (size_t)(rkc + 1) * 16));
    HIPCHK(f, take(seps, (size_t)nrec * 8));
    HIPCHK(f, take(small, FM_DBG_NCTR * 8));
    u64 *const d_start = reinterpret_cast<u64 *>(bits.p), *const d_node = d_start + nbw, *const d_out = d_node + nbw;
    u32 *const d_swpre = reinterpret_cast<u32 *>(wpre.p), *const d_owpre = d_swpre + nbw;
    u64 *const d_scsum = reinterpret_cast<u64 *>(csum.p), *const d_ocsum = d_scsum + rkc + 1;
    u64 *const d_seps = reinterpret_cast<u64 *>(seps.p), *const ctr = reinterpret_cast<u64 *>(small.p);
    std::vector<u64> hs(nrec);                                 // the separator positions
    for (u64 r = 0; r < nrec; r++) hs[r] = (r + 1 < nrec ? f->rec_starts[r + 1] : n) - 1;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < 5; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < 5; i++) HIPCHK(f, hipEventCreate(&ev[i]));
    HIPCHK(f, hipMemcpyAsync(d_seps, hs.data(), (size_t)nrec * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(bits.p, 0, (size_t)nbw * 24, f->stream));
    HIPCHK(f, hipMemsetAsync(ctr, 0, FM_DBG_NCTR * 8, f->stream));
    (void)hipEventRecord(ev[0], f->stream);
    k_fm_cdbg_rows<<<std::min<u32>(grid(n), 8192), 256, 0, f->stream>>>(f->esa_lcp.as<u32>(), f->esa_sa.as<u64>(), f->esa_da.as<u32>(),
                                                                        d_seps, nrec, n, k, d_start, d_node, d_out, ctr);
    k_fm_anc_count<<<(u32)rkc, FM_EX_CHUNK_WORDS, 0, f->stream>>>(d_start, nbw, d_swpre, d_scsum);
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(d_scsum, rkc, d_scsum + rkc);
    k_fm_anc_count<<<(u32)rkc, FM_EX_CHUNK_WORDS, 0, f->stream>>>(d_out, nbw, d_owpre, d_ocsum);
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(d_ocsum, rkc, d_ocsum + rkc);
    u64 hc[FM_DBG_NCTR], pieces = 0;
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(&pieces, d_scsum + rkc, 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    const u64 nodes = hc[FM_DBG_C_NODES], estr = hc[FM_DBG_C_ESTR];
    st.nodes = nodes; st.edge_strings = estr;
    if (!pieces || pieces > n || nodes > pieces) { f->err = "debwt_fm_cdbg: the start bits and their rank differ"; return DEBWT_EINTERNAL; }
    if (!nodes) {                                              // every record is shorter than k
        *sizes = debwt_fm_cdbg_sizes{0, 0, 0};
        st.ms_wall = (float)fm_ms_since(t0);
        return DEBWT_OK;
    }

    // pieces: first rows, degrees, links
    const u32 P = (u32)pieces;
    const u64 nbp = (pieces >> 6) + 1, rkp = (nbp + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;
    FmTmp lo, od, link, hasnext, s0, s1, l0, l1, hbits, hwpre, hcsum;
    HIPCHK(f, take(lo, (size_t)(pieces + 1) * 4));
    HIPCHK(f, take(od, (size_t)pieces * 4));
    HIPCHK(f, take(link, (size_t)pieces * 4));
    HIPCHK(f, take(hasnext, (size_t)pieces));
    HIPCHK(f, take(s0, (size_t)pieces * 16));
    HIPCHK(f, take(s1, (size_t)pieces * 16));
    HIPCHK(f, take(l0, (size_t)nodes * 4));
    HIPCHK(f, take(l1, (size_t)nodes * 4));
    HIPCHK(f, take(hbits, (size_t)nbp * 8));
    HIPCHK(f, take(hwpre, (size_t)nbp * 4));
    HIPCHK(f, take(hcsum, (size_t)(rkp + 1) * 8));
    u32 *const d_lo = reinterpret_cast<u32 *>(lo.p), *const d_od = reinterpret_cast<u32 *>(od.p), *const d_link = reinterpret_cast<u32 *>(link.p);
    u8 *const d_next = reinterpret_cast<u8 *>(hasnext.p);
    uint4 *const d_s[2] = {reinterpret_cast<uint4 *>(s0.p), reinterpret_cast<uint4 *>(s1.p)};
    u32 *const d_l[2] = {reinterpret_cast<u32 *>(l0.p), reinterpret_cast<u32 *>(l1.p)};
    const FmDbgBits S{d_start, d_swpre, d_scsum}, O{d_out, d_owpre, d_ocsum};
    const FmDbgBits H{reinterpret_cast<u64 *>(hbits.p), reinterpret_cast<u32 *>(hwpre.p), reinterpret_cast<u64 *>(hcsum.p)};
    k_fm_cdbg_lo<<<grid(n), 256, 0, f->stream>>>(S, n, P, d_lo);
    (void)hipEventRecord(ev[1], f->stream);
    HIPCHK(f, hipMemsetAsync(d_next, 0, (size_t)pieces, f->stream));
    k_fm_cdbg_degrees<<<few(pieces, 256), 256, 0, f->stream>>>(f->V, d_lo, P, d_node, S, O, d_od, d_link, ctr);
    k_fm_cdbg_links<<<few(pieces, 256), 256, 0, f->stream>>>(d_od, d_link, d_next, P, ctr);
    (void)hipEventRecord(ev[2], f->stream);
    k_fm_cdbg_init<<<few(pieces, FM_DBG_CHUNK), 256, 0, f->stream>>>(d_link, P, d_s[0], d_s[1], d_l[0], ctr);
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    if (hc[FM_DBG_C_BAD] || hc[FM_DBG_C_LIST] != hc[FM_DBG_C_LINKS] || hc[FM_DBG_C_LINKS] > nodes) {
        f->err = "debwt_fm_cdbg: " + std::to_string(hc[FM_DBG_C_BAD]) + " left extensions lie in no node, " +
                 std::to_string(hc[FM_DBG_C_LINKS]) + " links, " + std::to_string(hc[FM_DBG_C_LIST]) + " listed";
        return DEBWT_EINTERNAL;
    }
    const u64 links0 = hc[FM_DBG_C_LINKS];

    // ranking: the first phase ends when every listed node is finished or on a cycle that was found; the second ranks the
    // cycles after the cut
    u64 cnt = links0, target = links0, fin = 0, cyclen = 0, cycles = 0;
    int cur = 0, li = 0;
    for (int phase = 0; phase < 2 && cnt; phase++) {
        if (phase == 1) {
            HIPCHK(f, hipMemsetAsync(ctr + FM_DBG_C_LIST, 0, 3 * 8, f->stream));   // the list, finished, cycle lengths
            k_fm_cdbg_cut<<<few(cnt, FM_DBG_CHUNK), 256, 0, f->stream>>>(d_s[cur], d_link, d_od, d_next, d_l[li], cnt, d_s[0], d_s[1], d_l[1 - li], ctr);
            HIPCHK(f, hipMemcpyAsync(&cnt, ctr + FM_DBG_C_LIST, 8, hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;
            li ^= 1; target = cnt; fin = 0; cyclen = 0;
        }
        while (fin + cyclen < target) {
            u64 h4[4];
            HIPCHK(f, hipMemsetAsync(ctr + FM_DBG_C_LIST, 0, 8, f->stream));
            k_fm_cdbg_jump<<<few(cnt, FM_DBG_CHUNK), 256, 0, f->stream>>>(d_s[cur], d_s[1 - cur], d_l[li], cnt, d_l[1 - li], ctr);
            HIPCHK(f, hipMemcpyAsync(h4, ctr + FM_DBG_C_LIST, sizeof h4, hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;
            st.jump_rounds++; st.jump_steps += cnt; st.jump_wave_steps += (cnt + 63) / 64 * 64;
            if (h4[0] > cnt || st.jump_rounds > 80) { f->err = "debwt_fm_cdbg: the ranking does not end"; return DEBWT_EINTERNAL; }
            cnt = h4[0]; fin = h4[1]; cyclen = h4[2];
            if (phase == 0) cycles = h4[3];
            cur ^= 1; li ^= 1;
        }
        if (!cycles) break;
    }
    (void)hipEventRecord(ev[3], f->stream);
    if (cycles > links0) return DEBWT_EINTERNAL;
    const u64 links = links0 - cycles;                         // the link into the first node of a cycle is an edge
    HIPCHK(f, hipMemsetAsync(hbits.p, 0, (size_t)nbp * 8, f->stream));
    k_fm_cdbg_heads<<<std::min<u32>(grid(pieces), 8192), 256, 0, f->stream>>>(d_s[cur], d_od, d_link, P, reinterpret_cast<u64 *>(hbits.p), ctr);
    k_fm_anc_count<<<(u32)rkp, FM_EX_CHUNK_WORDS, 0, f->stream>>>(H.bits, nbp, reinterpret_cast<u32 *>(hwpre.p), reinterpret_cast<u64 *>(hcsum.p));
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(reinterpret_cast<u64 *>(hcsum.p), rkp, reinterpret_cast<u64 *>(hcsum.p) + rkp);
    u64 U = 0;
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(&U, H.csum + rkp, 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_nodes, ev[0], ev[1]);
    (void)hipEventElapsedTime(&st.ms_links, ev[1], ev[2]);
    (void)hipEventElapsedTime(&st.ms_rank, ev[2], ev[3]);
    if (U != nodes - links || estr < links) {
        f->err = "debwt_fm_cdbg: " + std::to_string(U) + " first nodes, " + std::to_string(nodes) + " nodes and " + std::to_string(links) + " links";
        return DEBWT_EINTERNAL;
    }
    const u64 E = estr - links, seq_bytes = nodes + U * ((u64)k - 1);
    st.unitigs = U; st.circular = cycles; st.links = links; st.edges = E; st.longest_nodes = hc[FM_DBG_C_LONGEST];
    st.seq_bytes = seq_bytes; st.rank_lines = hc[FM_DBG_C_LINES];
    *sizes = debwt_fm_cdbg_sizes{U, seq_bytes, E};
    if (unitig_capacity < U || seq_capacity < seq_bytes || edge_capacity < E) {
        st.ms_wall = (float)fm_ms_since(t0);
        f->err = "debwt_fm_cdbg: a capacity is below its size (" + std::to_string(U) + " unitigs, " + std::to_string(seq_bytes) +
                 " bytes, " + std::to_string(E) + " edges)";
        return DEBWT_ERANGE;
    }

    // the write pass
    const u64 ntiles = (U + FM_REC_TILE - 1) / FM_REC_TILE;
    FmTmp dun, dlen, dP, tsum, dseq, ka, kb, rws, dedge;
    HIPCHK(f, take(dun, (size_t)U * sizeof(debwt_fm_unitig)));
    HIPCHK(f, take(dlen, (size_t)U * 8));
    HIPCHK(f, take(dP, (size_t)U * 8));
    HIPCHK(f, take(tsum, (size_t)(ntiles + 1) * 8));
    HIPCHK(f, take(dseq, (size_t)seq_bytes));
    debwt_fm_unitig *const d_un = reinterpret_cast<debwt_fm_unitig *>(dun.p);
    u64 *const d_len = reinterpret_cast<u64 *>(dlen.p), *const d_P = reinterpret_cast<u64 *>(dP.p), *const d_tsum = reinterpret_cast<u64 *>(tsum.p);
    HIPCHK(f, hipMemsetAsync(dun.p, 0, (size_t)U * sizeof(debwt_fm_unitig), f->stream));
    k_fm_cdbg_unitigs<<<std::min<u32>(grid(pieces), 8192), 256, 0, f->stream>>>(d_s[cur], d_od, d_link, d_next, d_lo, P, H, U, k, d_un, d_len);
    k_fm_rec_tile_sums<u64><<<(u32)ntiles, FM_REC_TILE, 0, f->stream>>>(d_len, U, d_tsum);
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(d_tsum, ntiles, d_tsum + ntiles);
    k_fm_rec_scan<u64><<<(u32)ntiles, FM_REC_TILE, 0, f->stream>>>(d_len, U, d_tsum, d_P);
    k_fm_cdbg_seq<<<grid(pieces), 256, 0, f->stream>>>(d_s[cur], d_od, d_link, d_lo, P, H, U, k, d_P, d_len, f->esa_sa.as<u64>(),
                                                       f->text.as<u64>(), n, d_un, reinterpret_cast<u8 *>(dseq.p), seq_bytes);
    if (E) {
        const u32 ub = std::max<u32>(fm_bits_of(U - 1), 1);
        const size_t ws_bytes = radix_workspace_bytes(E);
        HIPCHK(f, take(ka, (size_t)E * 8));
        HIPCHK(f, take(kb, (size_t)E * 8));
        HIPCHK(f, take(rws, ws_bytes));
        HIPCHK(f, take(dedge, (size_t)E * sizeof(debwt_fm_cdbg_edge)));
        k_fm_cdbg_edges<<<few(pieces, 256), 256, 0, f->stream>>>(f->V, d_s[cur], d_od, d_link, d_lo, P, S, H, ub, reinterpret_cast<u64 *>(ka.p), E, ctr);
        const u64 *sorted = reinterpret_cast<u64 *>(ka.p);
        if (E >= 2) {
            RadixWorkspace ws{};
            ws.counts = reinterpret_cast<u32 *>(rws.p);        // chunk histograms only, as debwt_fm_records_build sorts
            hipError_t e = hipSuccess;
            sorted = radix_sort_bits(f->stream, reinterpret_cast<u64 *>(ka.p), reinterpret_cast<u64 *>(kb.p), E, 0, (int)(2 * ub), ws, &e);
            if (e != hipSuccess) { f->err = std::string("debwt_fm_cdbg: the key sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
        }
        k_fm_cdbg_edge_out<<<grid(E), 256, 0, f->stream>>>(sorted, E, ub, reinterpret_cast<debwt_fm_cdbg_edge *>(dedge.p));
        HIPCHK(f, hipMemcpyAsync(edges, dedge.p, (size_t)E * sizeof(debwt_fm_cdbg_edge), hipMemcpyDeviceToHost, f->stream));
    }
    (void)hipEventRecord(ev[4], f->stream);
    u64 total = 0;
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(&total, d_tsum + ntiles, 8, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(unitigs, dun.p, (size_t)U * sizeof(debwt_fm_unitig), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(seq, dseq.p, (size_t)seq_bytes, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_write, ev[3], ev[4]);
    st.rank_lines = hc[FM_DBG_C_LINES];
    if (total != seq_bytes || hc[FM_DBG_C_EDGES] != E) {
        f->err = "debwt_fm_cdbg: the write pass made " + std::to_string(total) + " bytes and " + std::to_string(hc[FM_DBG_C_EDGES]) +
                 " edges, the count said " + std::to_string(seq_bytes) + " and " + std::to_string(E);
        return DEBWT_EINTERNAL;
    }
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_cdbg_stats_get(const debwt_fm *f, debwt_fm_cdbg_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->dbg_stats;
    return DEBWT_OK;
}

// ---- compacted de Bruijn graph over both strands (fm_bicdbg_kernels.h) ------------------------------------------------
// The launches of debwt_fm_cdbg up to lo[], then mates, masks and links over the 2 x pieces oriented ids, the ranking
// rounds of debwt_fm_cdbg over those ids, the chain minima and the reported chains, and for a call that takes the graph
// the unitig records, the strings, and the edge keys sorted and made distinct.

static_assert(FM_BD_NCTR > FM_BD_C_CIRC && FM_BD_C_MATED > FM_DBG_C_EDGES, "the counters of both headers share one array");

extern "C" int debwt_fm_cdbg_both(debwt_fm *f, uint32_t k, uint32_t flags, debwt_fm_unitig *unitigs, uint64_t unitig_capacity,
                                  uint8_t *seq, uint64_t seq_capacity, debwt_fm_cdbg_edge *edges, uint64_t edge_capacity,
                                  debwt_fm_cdbg_sizes *sizes) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    if (!sizes) { f->err = "debwt_fm_cdbg_both: sizes must not be NULL"; return DEBWT_EINVAL; }
    if (!k) { f->err = "debwt_fm_cdbg_both: k must be at least 1"; return DEBWT_EINVAL; }
    if (!(k & 1u)) {
        f->err = "debwt_fm_cdbg_both: k must be odd (a k-mer of even length can be its own reverse complement, a node that is its own mirror)";
        return DEBWT_EINVAL;
    }
    if (flags) { f->err = "debwt_fm_cdbg_both: unknown flags"; return DEBWT_EINVAL; }
    if ((unitig_capacity && !unitigs) || (seq_capacity && !seq) || (edge_capacity && !edges)) {
        f->err = "debwt_fm_cdbg_both: an array is NULL with capacity > 0"; return DEBWT_EINVAL;
    }
    if (!f->has_esa || !f->esa_lcp.p || !f->esa_sa.p || !f->esa_da.p) {
        f->err = "debwt_fm_cdbg_both: no build holds lcp, sa and da (debwt_fm_esa_build with DEBWT_FM_ESA_SA | DEBWT_FM_ESA_DA)";
        return DEBWT_ESTATE;
    }
    if ((u64)k + 1 > f->esa_sum.cap) {
        f->err = "debwt_fm_cdbg_both: k + 1 is above the cap of the build (" + std::to_string(f->esa_sum.cap) + ")"; return DEBWT_EINVAL;
    }
    if (f->n >> 31) { f->err = "debwt_fm_cdbg_both: the index has 2^31 rows or more (an oriented id needs one more bit)"; return DEBWT_EINVAL; }
    f->bidbg_stats = debwt_fm_cdbg_both_stats{};
    debwt_fm_cdbg_both_stats &st = f->bidbg_stats;
    HIPCHK(f, hipSetDevice(f->device));
    int rc;
    if (!f->has_text && (rc = debwt_fm_restore_text(f))) return rc;
    const u64 n = f->n, nrec = f->nrec;
    auto grid = [](u64 m) { return (u32)std::min<u64>(std::max<u64>(grid_for(m, 256), 1), 1u << 20); };
    auto few = [](u64 m, u64 per) { return (u32)std::min<u64>(std::max<u64>((m + per - 1) / per, 1), 4096); };
    auto take = [&st](FmTmp &t, size_t bytes) { st.scratch_bytes += bytes; return hipMalloc(&t.p, std::max<size_t>(bytes, 8)); };

    // rows: as debwt_fm_cdbg
    const u64 nbw = (n >> 6) + 1, rkc = (nbw + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;
    FmTmp bits, wpre, csum, seps, small;
    HIPCHK(f, take(bits, (size_t)nbw * 24));
    HIPCHK(f, take(wpre, (size_t)nbw * 4));
    HIPCHK(f, take(csum, (size_t)(rkc + 1) * 8));
    HIPCHK(f, take(seps, (size_t)nrec * 8));
    HIPCHK(f, take(small, FM_BD_NCTR * 8));
    u64 *const d_start = reinterpret_cast<u64 *>(bits.p), *const d_node = d_start + nbw, *const d_out = d_node + nbw;
    u64 *const d_seps = reinterpret_cast<u64 *>(seps.p), *const ctr = reinterpret_cast<u64 *>(small.p);
    const FmDbgBits S{d_start, reinterpret_cast<u32 *>(wpre.p), reinterpret_cast<u64 *>(csum.p)};
    std::vector<u64> hs(nrec);                                 // the separator positions
    for (u64 r = 0; r < nrec; r++) hs[r] = (r + 1 < nrec ? f->rec_starts[r + 1] : n) - 1;
    const int NEV = 6;
    hipEvent_t ev[NEV] = {};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < NEV; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{ev};
    for (int i = 0; i < NEV; i++) HIPCHK(f, hipEventCreate(&ev[i]));
    HIPCHK(f, hipMemcpyAsync(d_seps, hs.data(), (size_t)nrec * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(bits.p, 0, (size_t)nbw * 24, f->stream));
    HIPCHK(f, hipMemsetAsync(ctr, 0, FM_BD_NCTR * 8, f->stream));
    (void)hipEventRecord(ev[0], f->stream);
    k_fm_cdbg_rows<<<std::min<u32>(grid(n), 8192), 256, 0, f->stream>>>(f->esa_lcp.as<u32>(), f->esa_sa.as<u64>(), f->esa_da.as<u32>(),
                                                                        d_seps, nrec, n, k, d_start, d_node, d_out, ctr);
    k_fm_anc_count<<<(u32)rkc, FM_EX_CHUNK_WORDS, 0, f->stream>>>(d_start, nbw, const_cast<u32 *>(S.wpre), const_cast<u64 *>(S.csum));
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(const_cast<u64 *>(S.csum), rkc, const_cast<u64 *>(S.csum) + rkc);
    u64 hc[FM_BD_NCTR], pieces = 0;
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(&pieces, S.csum + rkc, 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    const u64 present = hc[FM_DBG_C_NODES], estr = hc[FM_DBG_C_ESTR];
    st.present = present;
    if (!pieces || pieces > n || present > pieces) { f->err = "debwt_fm_cdbg_both: the start bits and their rank differ"; return DEBWT_EINTERNAL; }
    if (!present) {                                            // every record is shorter than k
        *sizes = debwt_fm_cdbg_sizes{0, 0, 0};
        st.ms_wall = (float)fm_ms_since(t0);
        return DEBWT_OK;
    }

    // oriented ids: mates, masks, links
    const u32 P = (u32)pieces;
    const u64 ids = 2 * pieces;
    const u64 nbp = (pieces >> 6) + 1, rkp = (nbp + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;
    FmTmp lo, mate, od, link, hasnext, s0, s1, l0, l1, cmin, wbits, wwpre, wcsum;
    HIPCHK(f, take(lo, (size_t)(pieces + 1) * 4));
    HIPCHK(f, take(mate, (size_t)pieces * 4));
    HIPCHK(f, take(od, (size_t)ids * 4));
    HIPCHK(f, take(link, (size_t)ids * 4));
    HIPCHK(f, take(hasnext, (size_t)ids));
    HIPCHK(f, take(s0, (size_t)ids * 16));
    HIPCHK(f, take(s1, (size_t)ids * 16));
    HIPCHK(f, take(l0, (size_t)present * 8));
    HIPCHK(f, take(l1, (size_t)present * 8));
    HIPCHK(f, take(cmin, (size_t)ids * 4));
    HIPCHK(f, take(wbits, (size_t)nbp * 8));
    HIPCHK(f, take(wwpre, (size_t)nbp * 4));
    HIPCHK(f, take(wcsum, (size_t)(rkp + 1) * 8));
    u32 *const d_lo = reinterpret_cast<u32 *>(lo.p), *const d_mate = reinterpret_cast<u32 *>(mate.p), *const d_od = reinterpret_cast<u32 *>(od.p);
    u32 *const d_link = reinterpret_cast<u32 *>(link.p), *const d_cmin = reinterpret_cast<u32 *>(cmin.p);
    u8 *const d_next = reinterpret_cast<u8 *>(hasnext.p);
    uint4 *const d_s[2] = {reinterpret_cast<uint4 *>(s0.p), reinterpret_cast<uint4 *>(s1.p)};
    u32 *const d_l[2] = {reinterpret_cast<u32 *>(l0.p), reinterpret_cast<u32 *>(l1.p)};
    const FmDbgBits W{reinterpret_cast<u64 *>(wbits.p), reinterpret_cast<u32 *>(wwpre.p), reinterpret_cast<u64 *>(wcsum.p)};
    k_fm_cdbg_lo<<<grid(n), 256, 0, f->stream>>>(S, n, P, d_lo);
    (void)hipEventRecord(ev[1], f->stream);
    k_fm_bicdbg_mates<<<grid(pieces), 256, 0, f->stream>>>(f->V, d_lo, P, d_node, S, f->esa_sa.as<u64>(), f->text.as<u64>(), k, d_mate, d_od, ctr);
    (void)hipEventRecord(ev[2], f->stream);
    HIPCHK(f, hipMemsetAsync(d_next, 0, (size_t)ids, f->stream));
    HIPCHK(f, hipMemsetAsync(d_link, 0xFF, (size_t)ids * 4, f->stream));
    HIPCHK(f, hipMemsetAsync(d_cmin, 0xFF, (size_t)ids * 4, f->stream));
    k_fm_bicdbg_degrees<<<few(pieces, 256), 256, 0, f->stream>>>(f->V, d_lo, P, d_node, S, f->esa_sa.as<u64>(), f->text.as<u64>(), k, d_mate, d_od, d_link, ctr);
    k_fm_bicdbg_links<<<few(ids, 256), 256, 0, f->stream>>>(d_od, d_mate, d_link, d_next, P, ctr);
    (void)hipEventRecord(ev[3], f->stream);
    k_fm_cdbg_init<<<few(ids, FM_DBG_CHUNK), 256, 0, f->stream>>>(d_link, (u32)ids, d_s[0], d_s[1], d_l[0], ctr);
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    const u64 mated = hc[FM_BD_C_MATED], valid = 2 * present - mated, oestr = hc[FM_BD_C_OESTR], links0 = hc[FM_DBG_C_LINKS];
    if (hc[FM_DBG_C_BAD] || mated > present || (mated & 1) || hc[FM_DBG_C_LIST] != links0 || links0 > valid || (links0 & 1) || oestr > 2 * estr) {
        f->err = "debwt_fm_cdbg_both: " + std::to_string(hc[FM_DBG_C_BAD]) + " mates or extensions lie in no node, " + std::to_string(mated) +
                 " mated, " + std::to_string(links0) + " links, " + std::to_string(hc[FM_DBG_C_LIST]) + " listed, " + std::to_string(oestr) +
                 " oriented edge strings";
        return DEBWT_EINTERNAL;
    }
    st.mated = mated; st.nodes = present - mated / 2; st.edge_strings = oestr; st.hairpins = hc[FM_BD_C_HAIRPINS];
    st.mate_steps = hc[FM_BD_C_STEPS];

    // ranking: the rounds of debwt_fm_cdbg over the oriented ids
    u64 cnt = links0, target = links0, fin = 0, cyclen = 0, cycles = 0;
    int cur = 0, li = 0;
    for (int phase = 0; phase < 2 && cnt; phase++) {
        if (phase == 1) {
            HIPCHK(f, hipMemsetAsync(ctr + FM_DBG_C_LIST, 0, 3 * 8, f->stream));   // the list, finished, cycle lengths
            k_fm_cdbg_cut<<<few(cnt, FM_DBG_CHUNK), 256, 0, f->stream>>>(d_s[cur], d_link, d_od, d_next, d_l[li], cnt, d_s[0], d_s[1], d_l[1 - li], ctr);
            HIPCHK(f, hipMemcpyAsync(&cnt, ctr + FM_DBG_C_LIST, 8, hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;
            li ^= 1; target = cnt; fin = 0; cyclen = 0;
        }
        while (fin + cyclen < target) {
            u64 h4[4];
            HIPCHK(f, hipMemsetAsync(ctr + FM_DBG_C_LIST, 0, 8, f->stream));
            k_fm_cdbg_jump<<<few(cnt, FM_DBG_CHUNK), 256, 0, f->stream>>>(d_s[cur], d_s[1 - cur], d_l[li], cnt, d_l[1 - li], ctr);
            HIPCHK(f, hipMemcpyAsync(h4, ctr + FM_DBG_C_LIST, sizeof h4, hipMemcpyDeviceToHost, f->stream));
            if ((rc = fm_sync(f))) return rc;
            st.jump_rounds++; st.jump_steps += cnt; st.jump_wave_steps += (cnt + 63) / 64 * 64;
            if (h4[0] > cnt || st.jump_rounds > 80) { f->err = "debwt_fm_cdbg_both: the ranking does not end"; return DEBWT_EINTERNAL; }
            cnt = h4[0]; fin = h4[1]; cyclen = h4[2];
            if (phase == 0) cycles = h4[3];
            cur ^= 1; li ^= 1;
        }
        if (!cycles) break;
    }
    (void)hipEventRecord(ev[4], f->stream);
    if (cycles > links0 || (cycles & 1)) { f->err = "debwt_fm_cdbg_both: " + std::to_string(cycles) + " oriented cycles"; return DEBWT_EINTERNAL; }
    const u64 links = (links0 - cycles) / 2;                   // member links of the reported unitigs; the cut links are edges
    HIPCHK(f, hipMemsetAsync(wbits.p, 0, (size_t)nbp * 8, f->stream));
    k_fm_bicdbg_mins<<<std::min<u32>(grid(ids), 8192), 256, 0, f->stream>>>(d_s[cur], d_od, P, d_cmin);
    k_fm_bicdbg_pairs<<<few(ids, 256), 256, 0, f->stream>>>(d_s[cur], d_od, d_link, d_mate, d_cmin, P, const_cast<u64 *>(W.bits), ctr);
    k_fm_anc_count<<<(u32)rkp, FM_EX_CHUNK_WORDS, 0, f->stream>>>(W.bits, nbp, const_cast<u32 *>(W.wpre), const_cast<u64 *>(W.csum));
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(const_cast<u64 *>(W.csum), rkp, const_cast<u64 *>(W.csum) + rkp);
    u64 U = 0;
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(&U, W.csum + rkp, 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_nodes, ev[0], ev[1]);
    (void)hipEventElapsedTime(&st.ms_mates, ev[1], ev[2]);
    (void)hipEventElapsedTime(&st.ms_links, ev[2], ev[3]);
    (void)hipEventElapsedTime(&st.ms_rank, ev[3], ev[4]);
    if (hc[FM_DBG_C_BAD] || 2 * U != valid - 2 * links || hc[FM_BD_C_REPORTED] != U || oestr < 2 * links || (hc[FM_BD_C_CIRC] * 2 != cycles)) {
        f->err = "debwt_fm_cdbg_both: " + std::to_string(U) + " reported unitigs, " + std::to_string(hc[FM_BD_C_REPORTED]) + " reported chains, " +
                 std::to_string(valid) + " oriented nodes, " + std::to_string(links) + " links, " + std::to_string(cycles) + " oriented cycles";
        return DEBWT_EINTERNAL;
    }
    const u64 E = oestr - 2 * links, seq_bytes = st.nodes + U * ((u64)k - 1);
    st.unitigs = U; st.circular = cycles / 2; st.links = links; st.edges = E; st.longest_nodes = hc[FM_DBG_C_LONGEST];
    st.seq_bytes = seq_bytes; st.rank_lines = hc[FM_DBG_C_LINES];
    *sizes = debwt_fm_cdbg_sizes{U, seq_bytes, E};
    if (unitig_capacity < U || seq_capacity < seq_bytes || edge_capacity < E) {
        st.ms_wall = (float)fm_ms_since(t0);
        f->err = "debwt_fm_cdbg_both: a capacity is below its size (" + std::to_string(U) + " unitigs, " + std::to_string(seq_bytes) +
                 " bytes, " + std::to_string(E) + " edges)";
        return DEBWT_ERANGE;
    }

    // the write pass
    const u64 ntiles = (U + FM_REC_TILE - 1) / FM_REC_TILE;
    FmTmp dun, dlen, dP, tsum, dseq, ka, kb, rws, dedge, qbits, qwpre, qcsum;
    HIPCHK(f, take(dun, (size_t)U * sizeof(debwt_fm_unitig)));
    HIPCHK(f, take(dlen, (size_t)U * 8));
    HIPCHK(f, take(dP, (size_t)U * 8));
    HIPCHK(f, take(tsum, (size_t)(ntiles + 1) * 8));
    HIPCHK(f, take(dseq, (size_t)seq_bytes));
    debwt_fm_unitig *const d_un = reinterpret_cast<debwt_fm_unitig *>(dun.p);
    u64 *const d_len = reinterpret_cast<u64 *>(dlen.p), *const d_P = reinterpret_cast<u64 *>(dP.p), *const d_tsum = reinterpret_cast<u64 *>(tsum.p);
    HIPCHK(f, hipMemsetAsync(dun.p, 0, (size_t)U * sizeof(debwt_fm_unitig), f->stream));
    k_fm_bicdbg_unitigs<<<std::min<u32>(grid(ids), 8192), 256, 0, f->stream>>>(d_s[cur], d_od, d_mate, d_next, d_lo, d_cmin, P, W, U, k, d_un, d_len);
    k_fm_rec_tile_sums<u64><<<(u32)ntiles, FM_REC_TILE, 0, f->stream>>>(d_len, U, d_tsum);
    k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(d_tsum, ntiles, d_tsum + ntiles);
    k_fm_rec_scan<u64><<<(u32)ntiles, FM_REC_TILE, 0, f->stream>>>(d_len, U, d_tsum, d_P);
    k_fm_bicdbg_seq<<<grid(ids), 256, 0, f->stream>>>(d_s[cur], d_od, d_lo, d_cmin, P, W, U, k, d_P, d_len, f->esa_sa.as<u64>(),
                                                      f->text.as<u64>(), n, d_un, reinterpret_cast<u8 *>(dseq.p), seq_bytes);
    u64 M = 0, distinct = 0;
    if (E) {
        const u64 cap = 2 * estr;                              // every forward edge string and its mirror, at most
        const u32 ub = std::max<u32>(fm_bits_of(2 * U - 1), 1);
        HIPCHK(f, take(ka, (size_t)cap * 8));
        HIPCHK(f, take(kb, (size_t)cap * 8));
        HIPCHK(f, take(rws, radix_workspace_bytes(cap)));
        HIPCHK(f, take(dedge, (size_t)E * sizeof(debwt_fm_cdbg_edge)));
        k_fm_bicdbg_edges<<<few(pieces, 256), 256, 0, f->stream>>>(f->V, d_s[cur], d_od, d_mate, d_link, d_lo, d_cmin, P, d_node, S, W, ub,
                                                                  reinterpret_cast<u64 *>(ka.p), cap, ctr);
        HIPCHK(f, hipMemcpyAsync(&M, ctr + FM_DBG_C_EDGES, 8, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
        if (M < E || M > cap) {
            f->err = "debwt_fm_cdbg_both: " + std::to_string(M) + " edge keys for " + std::to_string(E) + " edges and room for " + std::to_string(cap);
            return DEBWT_EINTERNAL;
        }
        const u64 *sorted = reinterpret_cast<u64 *>(ka.p);
        if (M >= 2) {
            RadixWorkspace ws{};
            ws.counts = reinterpret_cast<u32 *>(rws.p);        // chunk histograms only, as debwt_fm_records_build sorts
            hipError_t e = hipSuccess;
            sorted = radix_sort_bits(f->stream, reinterpret_cast<u64 *>(ka.p), reinterpret_cast<u64 *>(kb.p), M, 0, (int)(2 * ub), ws, &e);
            if (e != hipSuccess) { f->err = std::string("debwt_fm_cdbg_both: the key sort: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
        }
        const u64 nbq = (M >> 6) + 1, rkq = (nbq + FM_EX_CHUNK_WORDS - 1) / FM_EX_CHUNK_WORDS;
        HIPCHK(f, take(qbits, (size_t)nbq * 8));
        HIPCHK(f, take(qwpre, (size_t)nbq * 4));
        HIPCHK(f, take(qcsum, (size_t)(rkq + 1) * 8));
        const FmDbgBits Q{reinterpret_cast<u64 *>(qbits.p), reinterpret_cast<u32 *>(qwpre.p), reinterpret_cast<u64 *>(qcsum.p)};
        HIPCHK(f, hipMemsetAsync(qbits.p, 0, (size_t)nbq * 8, f->stream));
        k_fm_bicdbg_uniq<<<std::min<u32>(grid(M), 8192), 256, 0, f->stream>>>(sorted, M, const_cast<u64 *>(Q.bits));
        k_fm_anc_count<<<(u32)rkq, FM_EX_CHUNK_WORDS, 0, f->stream>>>(Q.bits, nbq, const_cast<u32 *>(Q.wpre), const_cast<u64 *>(Q.csum));
        k_fm_anc_scan<<<1, 1024, 0, f->stream>>>(const_cast<u64 *>(Q.csum), rkq, const_cast<u64 *>(Q.csum) + rkq);
        k_fm_bicdbg_edge_out<<<grid(M), 256, 0, f->stream>>>(sorted, M, Q, ub, E, reinterpret_cast<debwt_fm_cdbg_edge *>(dedge.p));
        HIPCHK(f, hipMemcpyAsync(&distinct, Q.csum + rkq, 8, hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
        if (distinct != E) {
            f->err = "debwt_fm_cdbg_both: " + std::to_string(distinct) + " distinct edge keys, the count said " + std::to_string(E);
            return DEBWT_EINTERNAL;
        }
        HIPCHK(f, hipMemcpyAsync(edges, dedge.p, (size_t)E * sizeof(debwt_fm_cdbg_edge), hipMemcpyDeviceToHost, f->stream));
    }
    (void)hipEventRecord(ev[5], f->stream);
    u64 total = 0;
    HIPCHK(f, hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(&total, d_tsum + ntiles, 8, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    if (total != seq_bytes) {
        f->err = "debwt_fm_cdbg_both: the write pass made " + std::to_string(total) + " bytes, the count said " + std::to_string(seq_bytes);
        return DEBWT_EINTERNAL;
    }
    HIPCHK(f, hipMemcpyAsync(unitigs, dun.p, (size_t)U * sizeof(debwt_fm_unitig), hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(seq, dseq.p, (size_t)seq_bytes, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    (void)hipEventElapsedTime(&st.ms_write, ev[4], ev[5]);
    st.rank_lines = hc[FM_DBG_C_LINES]; st.edge_keys = M;
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_cdbg_both_stats_get(const debwt_fm *f, debwt_fm_cdbg_both_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->bidbg_stats;
    return DEBWT_OK;
}

// ---- string graph of the indexed records, on one strand or on both (fm_graph_kernels.h, fm_bigraph_kernels.h) --------
// debwt_fm_string_graph and debwt_fm_string_graph_both share one host path: fm_graph_found, then fm_graph_finish.
// States come from one backward search per record over the attached text.  The kept records then go through the overlap
// walk in the batches of debwt_fm_overlaps, unpacked from the text on the device, on one strand or on both.  A batch's hits
// are expanded at most DEBWT_FM_OVERLAP_HITS at a launch into o_hits and packed to 8 bytes each into the batch's raw list
// (g_raw), which has one segment per record (its hits) or three (strand-0 hits, located tail seeds, strand-1 hits); the
// longest entry per (segment, target) is flagged, and the flagged ones are appended to g_edges, grown by doubling.  Per
// batch the run, hit and edge counts of its records reach the host, which lays the lists out; the edges stay in HBM until
// the reduction has run over them.

namespace {

static_assert(sizeof(debwt_fm_edge) == sizeof(FmEdge), "the graph kernels write debwt_fm_edge as FmEdge");
static_assert((int)FM_BG_BADLEN == (int)FM_GR_BADLEN && (int)FM_BG_NCTR == (int)FM_GR_NCTR, "g_ctr and b_ctr are read back alike");

// a builder's statistics struct says which of the two it is; both structs name the fields they share alike
template <class St> constexpr bool fm_graph_both = std::is_same<St, debwt_fm_graph_both_stats>::value;

struct FmGraphTimer {                                  // a timed stretch of the stream: begin(), launches, end(&ms)
    debwt_fm *f;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit FmGraphTimer(debwt_fm *f_) : f(f_) {}
    ~FmGraphTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    int init() {
        HIPCHK(f, hipEventCreate(&e0));
        HIPCHK(f, hipEventCreate(&e1));
        return DEBWT_OK;
    }
    void begin() { (void)hipEventRecord(e0, f->stream); }
    int end(float *acc) {
        (void)hipEventRecord(e1, f->stream);
        int rc = fm_sync(f);
        if (rc) return rc;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *acc += ms;
        return DEBWT_OK;
    }
};

// room for nedges edges in g_edges, the first `have` of them kept
int fm_graph_reserve(debwt_fm *f, const char *who, u64 have, u64 nedges) {
    const size_t need = (size_t)std::max<u64>(nedges, 1) * sizeof(FmEdge);
    if (need <= f->g_edges.cap) return DEBWT_OK;
    HIPCHK(f, hipStreamSynchronize(f->stream));
    size_t want = std::max(need, f->g_edges.cap * 2);
    void *p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError();
        want = need;
        if (hipMalloc(&p, want) != hipSuccess) {
            (void)hipGetLastError();
            f->err = std::string(who) + ": the edge list does not fit in device memory (" + std::to_string(nedges) +
                     " edges so far, 8 bytes each)";
            return DEBWT_ENOMEM;
        }
    }
    if (have) {
        hipError_t e = hipMemcpyAsync(p, f->g_edges.p, (size_t)have * sizeof(FmEdge), hipMemcpyDeviceToDevice, f->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
        if (e != hipSuccess) { (void)hipFree(p); f->err = std::string("hipMemcpyAsync: ") + hipGetErrorString(e); return DEBWT_EDEVICE; }
    }
    if (f->g_edges.p) (void)hipFree(f->g_edges.p);
    f->g_edges.p = p; f->g_edges.cap = want;
    return DEBWT_OK;
}

// the keep bytes of definition 3 for the lists in g_eoff / `edges` (device), into g_keep; st counts the launch, the lists
// searched, the reducible edges and the time
template <class St>
int fm_graph_reduce(debwt_fm *f, St &st, FmGraphTimer &tm, u64 nnodes, const FmEdge *edges, u64 nedges) {
    FM_ENSURE(f, f->g_keep, (size_t)nedges);
    FM_ENSURE(f, f->g_ctr, FM_GR_NCTR * 8);
    HIPCHK(f, hipMemsetAsync(f->g_ctr.p, 0, FM_GR_NCTR * 8, f->stream));
    tm.begin();
    k_fm_graph_reduce<<<grid_for(nedges, 256), 256, 0, f->stream>>>(f->g_eoff.as<u64>(), nnodes, edges, nedges, f->g_len.as<u64>(),
                                                                    f->g_keep.as<u8>(), f->g_ctr.as<u64>());
    u64 h[FM_GR_NCTR];
    HIPCHK(f, hipMemcpyAsync(h, f->g_ctr.p, sizeof h, hipMemcpyDeviceToHost, f->stream));
    int rc = tm.end(&st.ms_reduce);
    if (rc) return rc;
    st.launches++;
    st.lookups = h[FM_GR_LOOKUPS]; st.reducible = h[FM_GR_REDUCIBLE];
    return DEBWT_OK;
}

// the text and the overlap table in place; coff, the bases before each record, on the host and in g_coff
int fm_graph_text(debwt_fm *f, const char *who, std::vector<u64> &coff) {
    const u64 nrec = f->nrec;
    int rc;
    if (!f->has_text && (rc = debwt_fm_restore_text(f))) return rc;
    if ((rc = fm_overlap_table(f))) return rc;
    coff.resize(nrec + 1);
    for (u64 i = 0; i < nrec; i++) coff[i] = f->rec_starts[i] - i;
    coff[nrec] = f->n - nrec;
    for (u64 i = 0; i < nrec; i++)
        if ((coff[i + 1] - coff[i]) >> 32) { f->err = std::string(who) + ": a record of 2^32 bases or more"; return DEBWT_EINVAL; }
    FM_ENSURE(f, f->g_coff, (size_t)(nrec + 1) * 8);
    HIPCHK(f, hipMemcpyAsync(f->g_coff.p, coff.data(), (nrec + 1) * 8, hipMemcpyHostToDevice, f->stream));
    return DEBWT_OK;
}

// The states and the edges found, for either builder; eoff has NK nrec + 1 entries.
// One strand: state per record (host and g_state), one segment per record, so eoff is edge_offsets and g_edges holds E.
// Both strands: state per node (host and b_state), self-rc flags (b_self), three segments per record, so record i's ++, +-
// and -+ edges stand in [eoff[3i], eoff[3i + 1]), [eoff[3i + 1], eoff[3i + 2]), [eoff[3i + 2], eoff[3i + 3]) of g_edges (A).
// A batch has NS np items (item g: record p0 + g % np on strand g / np) and NK np segments.  On one strand the three base
// tables of a batch coincide -- hits in item order, hits in (record, strand) order, raw segments -- and g_hbase is all three.
template <class St>
int fm_graph_found(debwt_fm *f, St &st, const char *who, FmGraphTimer &tm, u32 min_overlap, uint8_t *state, uint64_t *eoff) {
    constexpr bool both = fm_graph_both<St>;
    constexpr u64 NS = both ? 2 : 1, NK = both ? 3 : 1;        // strands per record, segments per record
    const u64 nrec = f->nrec;
    std::vector<u64> coff;
    int rc = fm_graph_text(f, who, coff);
    if (rc) return rc;
    DevBuf &ctr = both ? f->b_ctr : f->g_ctr;
    DevBuf &d_ihb = both ? f->o_hbase : f->g_hbase, &d_whb = both ? f->b_whb : f->g_hbase, &d_seg = both ? f->b_rawbase : f->g_hbase;
    FM_ENSURE(f, ctr, FM_GR_NCTR * 8);
    HIPCHK(f, hipMemsetAsync(ctr.p, 0, FM_GR_NCTR * 8, f->stream));
    if constexpr (both) {
        std::vector<u8> selfrc(nrec, 0);
        FM_ENSURE(f, f->b_state, (size_t)nrec * 2);
        FM_ENSURE(f, f->b_self, (size_t)nrec);
        tm.begin();
        k_fm_bigraph_state<<<grid_for(nrec, 256), 256, 0, f->stream>>>(f->V, f->text.as<u64>(), f->g_coff.as<u64>(), f->o_table.as<FmOvlRec>(),
                                                                       nrec, f->b_state.as<u8>(), f->b_self.as<u8>());
        HIPCHK(f, hipMemcpyAsync(state, f->b_state.p, nrec * 2, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(f, hipMemcpyAsync(selfrc.data(), f->b_self.p, nrec, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_walk))) return rc;
        for (u64 i = 0; i < nrec; i++)
            if (state[2 * i] == 0) st.selfrc += selfrc[i];
    } else {
        FM_ENSURE(f, f->g_state, (size_t)nrec);
        tm.begin();
        k_fm_graph_state<<<grid_for(nrec, 256), 256, 0, f->stream>>>(f->V, f->text.as<u64>(), f->g_coff.as<u64>(),
                                                                     f->o_table.as<FmOvlRec>(), nrec, f->g_state.as<u8>());
        HIPCHK(f, hipMemcpyAsync(state, f->g_state.p, nrec, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_walk))) return rc;
    }
    st.launches++;
    st.records = nrec;
    for (u64 i = 0; i < nrec; i++) {
        if (state[NS * i] == 0) st.kept++;
        else if (state[NS * i] == 1) st.duplicates++;
        else st.contained++;
    }
    const u64 slots = fm_env_u64("DEBWT_FM_OVERLAP_SLOTS", FM_OVL_SLOTS);
    const u64 limit = std::max<u64>(fm_env_u64("DEBWT_FM_OVERLAP_HITS", FM_OVL_HITS), 1);
    auto worst = [&](u64 i) {                                  // run slots of record i on one strand
        const u64 m = coff[i + 1] - coff[i];
        return state[NS * i] == 0 && m >= min_overlap ? m - min_overlap + 1 : 0;
    };
    std::vector<u64> slot, rbase, ihb, whb, rawbase, tbase, oseg, nh, tc;
    std::vector<u32> nr, deg;
    eoff[0] = 0;
    for (u64 p0 = 0; p0 < nrec;) {
        u64 p1 = p0 + 1, ws = NS * worst(p0);                  // at least one record, however long
        while (p1 < nrec && p1 - p0 < FM_BATCH_PATTERNS && coff[p1 + 1] - coff[p0] <= FM_BATCH_CHARS && ws + NS * worst(p1) <= slots)
            ws += NS * worst(p1++);
        const u64 np = p1 - p0, nit = NS * np, nseg = NK * np, bytes = coff[p1] - coff[p0];
        for (u64 k = NK * p0; k < NK * p1; k++) eoff[k + 1] = eoff[k];
        if (!ws) { p0 = p1; continue; }                        // no kept record long enough: no edges
        slot.resize(nit + 1);
        slot[0] = 0;
        for (u64 g = 0; g < nit; g++) slot[g + 1] = slot[g] + worst(p0 + g % np);
        FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(bytes, 1));
        FM_ENSURE(f, f->o_slot, (size_t)(nit + 1) * 8);
        FM_ENSURE(f, f->o_nruns, (size_t)nit * 4);
        FM_ENSURE(f, f->o_nhits, (size_t)nit * 8);
        FM_ENSURE(f, f->o_runs, (size_t)ws * sizeof(FmOvlRun));
        FM_ENSURE(f, f->s_ctr, 64);
        HIPCHK(f, hipMemcpyAsync(f->o_slot.p, slot.data(), (nit + 1) * 8, hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemsetAsync(f->s_ctr.p, 0, 32, f->stream));
        tm.begin();
        k_fm_graph_unpack<<<grid_for(bytes, 256), 256, 0, f->stream>>>(f->text.as<u64>(), f->g_coff.as<u64>(), p0, np, bytes,
                                                                       f->q_chars.as<u8>());
        k_fm_overlap_walk<<<grid_for(nit, 256), 256, 0, f->stream>>>(f->V, f->q_chars.as<u8>(), f->g_coff.as<u64>() + p0, coff[p0], np,
                                                                     nit, min_overlap, f->o_slot.as<u64>(), f->o_runs.as<FmOvlRun>(),
                                                                     f->o_nruns.as<u32>(), f->o_nhits.as<u64>(), f->s_ctr.as<u64>());
        nr.resize(nit); nh.resize(nit);
        HIPCHK(f, hipMemcpyAsync(nr.data(), f->o_nruns.p, nit * 4, hipMemcpyDeviceToHost, f->stream));
        HIPCHK(f, hipMemcpyAsync(nh.data(), f->o_nhits.p, nit * 8, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_walk))) return rc;
        st.launches += 2;
        if constexpr (both) {                                  // the tail seeds of the batch and their row counts
            FM_ENSURE(f, f->b_row, (size_t)np * 8);
            FM_ENSURE(f, f->b_cnt, (size_t)np * 8);
            tc.resize(np);
            tm.begin();
            k_fm_bigraph_seed<<<grid_for(np, 256), 256, 0, f->stream>>>(f->V, f->text.as<u64>(), f->g_coff.as<u64>(), f->b_state.as<u8>(), p0,
                                                                        np, min_overlap, f->b_row.as<u64>(), f->b_cnt.as<u64>(),
                                                                        f->b_ctr.as<u64>());
            HIPCHK(f, hipMemcpyAsync(tc.data(), f->b_cnt.p, np * 8, hipMemcpyDeviceToHost, f->stream));
            if ((rc = tm.end(&st.ms_tail))) return rc;
            st.launches++;
        }
        // runs in item order; walk hits in item order (ihb) and in (record, strand) order (whb); raw segments by (record, kind)
        rbase.resize(nit); whb.resize(nit + 1);
        if constexpr (both) { ihb.resize(nit); rawbase.resize(nseg + 1); tbase.resize(np + 1); }
        u64 nruns = 0, nhits = 0, ntail = 0, nraw = 0;
        for (u64 j = 0; j < np; j++) {
            for (u64 s = 0; s < NS; s++) {
                const u64 g = s * np + j;
                if (nr[g] > slot[g + 1] - slot[g]) { f->err = std::string(who) + ": a record wrote more runs than its slots"; return DEBWT_EINTERNAL; }
                rbase[g] = nruns; whb[NS * j + s] = nhits;
                if constexpr (both) ihb[g] = nhits;
                nruns += nr[g]; nhits += nh[g];
            }
            if constexpr (both) {
                rawbase[3 * j] = nraw; nraw += nh[j];
                rawbase[3 * j + 1] = nraw; nraw += tc[j];
                rawbase[3 * j + 2] = nraw; nraw += nh[np + j];
                tbase[j] = ntail; ntail += tc[j];
            }
        }
        whb[nit] = nhits;
        st.hits += nhits;
        if constexpr (both) { rawbase[nseg] = nraw; tbase[np] = ntail; st.seed_rows += ntail; }
        else nraw = nhits;
        if (!nraw) { p0 = p1; continue; }
        const u64 chunk = std::min(std::max(nhits, ntail), limit);
        FM_ENSURE(f, f->o_rbase, (size_t)nit * 8);
        FM_ENSURE(f, d_whb, (size_t)(nit + 1) * 8);
        FM_ENSURE(f, f->o_cruns, (size_t)std::max<u64>(nruns, 1) * sizeof(FmOvlRun));
        FM_ENSURE(f, f->o_rout, (size_t)std::max<u64>(nruns, 1) * 8);
        FM_ENSURE(f, f->o_hits, (size_t)chunk * sizeof(uint4));
        FM_ENSURE(f, f->g_raw, (size_t)nraw * sizeof(FmEdge));
        FM_ENSURE(f, f->g_flag, (size_t)nraw);
        FM_ENSURE(f, f->g_deg, (size_t)nseg * 4);
        FM_ENSURE(f, f->g_oseg, (size_t)(nseg + 1) * 8);
        HIPCHK(f, hipMemcpyAsync(f->o_rbase.p, rbase.data(), nit * 8, hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemcpyAsync(d_whb.p, whb.data(), (nit + 1) * 8, hipMemcpyHostToDevice, f->stream));
        if constexpr (both) {
            FM_ENSURE(f, f->o_hbase, (size_t)nit * 8);
            FM_ENSURE(f, f->b_rawbase, (size_t)(nseg + 1) * 8);
            FM_ENSURE(f, f->b_tbase, (size_t)(np + 1) * 8);
            FM_ENSURE(f, f->b_pos, (size_t)chunk * 8);
            st.scratch_bytes = std::max<u64>(st.scratch_bytes, bytes + ws * sizeof(FmOvlRun) + np * 120 + nruns * 24 + chunk * 24 + nraw * 9);
            HIPCHK(f, hipMemcpyAsync(f->o_hbase.p, ihb.data(), nit * 8, hipMemcpyHostToDevice, f->stream));
            HIPCHK(f, hipMemcpyAsync(f->b_rawbase.p, rawbase.data(), (nseg + 1) * 8, hipMemcpyHostToDevice, f->stream));
            HIPCHK(f, hipMemcpyAsync(f->b_tbase.p, tbase.data(), (np + 1) * 8, hipMemcpyHostToDevice, f->stream));
        } else {
            st.scratch_bytes = std::max<u64>(st.scratch_bytes, bytes + ws * sizeof(FmOvlRun) + np * 48 + nruns * 24 + chunk * 16 + nhits * 9);
        }
        if (nhits) {
            tm.begin();
            k_fm_overlap_compact<<<grid_for(nit, 256), 256, 0, f->stream>>>(f->g_coff.as<u64>() + p0, f->o_slot.as<u64>(), f->o_nruns.as<u32>(),
                                                                            f->o_rbase.as<u64>(), d_ihb.as<u64>(), np, nit,
                                                                            f->o_runs.as<FmOvlRun>(), f->o_cruns.as<FmOvlRun>(),
                                                                            f->o_rout.as<u64>());
            st.launches++;
            for (u64 g0 = 0; g0 < nhits; g0 += chunk) {
                const u64 cnt = std::min(nhits - g0, chunk);
                if (g0) tm.begin();
                k_fm_overlap_expand<<<grid_for(cnt, 256), 256, 0, f->stream>>>(f->o_cruns.as<FmOvlRun>(), f->o_rout.as<u64>(), nruns,
                                                                               f->o_table.as<FmOvlRec>(), g0, cnt, f->o_hits.as<uint4>());
                if ((rc = tm.end(&st.ms_walk))) return rc;
                tm.begin();
                if constexpr (both)
                    k_fm_bigraph_pack<<<grid_for(cnt, 256), 256, 0, f->stream>>>(f->o_hits.as<uint4>(), g0, cnt, f->b_whb.as<u64>(),
                                                                                 f->b_rawbase.as<u64>(), p0, np, f->b_state.as<u8>(),
                                                                                 f->b_self.as<u8>(), f->g_raw.as<FmEdge>(), f->b_ctr.as<u64>());
                else
                    k_fm_graph_pack<<<grid_for(cnt, 256), 256, 0, f->stream>>>(f->o_hits.as<uint4>(), g0, cnt, f->g_hbase.as<u64>(), p0, np,
                                                                               f->g_state.as<u8>(), f->g_raw.as<FmEdge>(), f->g_ctr.as<u64>());
                if ((rc = tm.end(&st.ms_build))) return rc;
                st.launches += 2;
            }
        }
        if constexpr (both)
            for (u64 g0 = 0; g0 < ntail; g0 += chunk) {        // the seeds' rows are the runs of the locate kernel
                const u64 cnt = std::min(ntail - g0, chunk);
                tm.begin();
                k_fm_locate<<<grid_for(cnt, 256), 256, 0, f->stream>>>(f->V, f->sa.as<u64>(), f->sh, f->b_row.as<u64>(), f->b_tbase.as<u64>(), np,
                                                                      g0, cnt, f->b_pos.as<u64>());
                k_fm_bigraph_tail<<<grid_for(cnt, 256), 256, 0, f->stream>>>(f->text.as<u64>(), f->g_coff.as<u64>(), nrec, f->b_pos.as<u64>(), g0,
                                                                             cnt, f->b_tbase.as<u64>(), f->b_rawbase.as<u64>(), p0, np,
                                                                             min_overlap, f->b_state.as<u8>(), f->b_self.as<u8>(),
                                                                             f->g_raw.as<FmEdge>(), f->b_ctr.as<u64>());
                if ((rc = tm.end(&st.ms_tail))) return rc;
                st.launches += 2;
            }
        tm.begin();
        if constexpr (both)                                    // not for one strand: it reads a whole segment per entry
            k_fm_bigraph_longest<<<grid_for(nraw, 256), 256, 0, f->stream>>>(f->g_raw.as<FmEdge>(), d_seg.as<u64>(), nseg, nraw,
                                                                             f->g_flag.as<u8>());
        else
            k_fm_graph_longest<<<grid_for(nraw, 256), 256, 0, f->stream>>>(f->g_raw.as<FmEdge>(), d_seg.as<u64>(), nseg, nraw,
                                                                           f->g_flag.as<u8>());
        k_fm_graph_degree<<<grid_for(nseg, 256), 256, 0, f->stream>>>(f->g_flag.as<u8>(), d_seg.as<u64>(), nseg, f->g_deg.as<u32>());
        deg.resize(nseg);
        HIPCHK(f, hipMemcpyAsync(deg.data(), f->g_deg.p, nseg * 4, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_build))) return rc;
        st.launches += 2;
        oseg.resize(nseg + 1);
        for (u64 k = 0; k < nseg; k++) { oseg[k] = eoff[NK * p0 + k]; eoff[NK * p0 + k + 1] = eoff[NK * p0 + k] + deg[k]; }
        oseg[nseg] = eoff[NK * p1];
        if (eoff[NK * p1] > eoff[NK * p0]) {
            if ((rc = fm_graph_reserve(f, who, eoff[NK * p0], eoff[NK * p1]))) return rc;
            HIPCHK(f, hipMemcpyAsync(f->g_oseg.p, oseg.data(), (nseg + 1) * 8, hipMemcpyHostToDevice, f->stream));
            tm.begin();
            k_fm_graph_scatter<<<grid_for(nraw, 256), 256, 0, f->stream>>>(f->g_raw.as<FmEdge>(), f->g_flag.as<u8>(), d_seg.as<u64>(),
                                                                           f->g_oseg.as<u64>(), nseg, nraw, f->g_edges.as<FmEdge>());
            if ((rc = tm.end(&st.ms_build))) return rc;     // oseg is host memory
            st.launches++;
        }
        p0 = p1;
    }
    u64 h[FM_GR_NCTR];
    HIPCHK(f, hipMemcpyAsync(h, ctr.p, sizeof h, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    if (h[FM_GR_BADLEN]) {
        f->err = std::string(who) + ": " + std::to_string(h[FM_GR_BADLEN]) + " overlaps between kept records cover one of them whole";
        return DEBWT_EINTERNAL;
    }
    if constexpr (both) { st.seeds = h[FM_BG_SEEDS]; st.tail_hits = h[FM_BG_TAILS]; }
    return DEBWT_OK;
}

// The end of either builder.  E is in g_edges, its nnodes lists in edge_offsets.  Unless all edges are asked for: the keep
// bytes of the reduction, the degrees of the kept edges, the new offsets, the kept edges scattered into g_out, as a batch's
// flagged entries were into g_edges.  Then the capacity protocol and the copy to the host.  The node lengths are computed
// here, and only when the reduction runs.
template <class St>
int fm_graph_finish(debwt_fm *f, St &st, const char *who, FmGraphTimer &tm, u32 flags, u64 nnodes, uint64_t *edge_offsets,
                    debwt_fm_edge *edges, u64 capacity) {
    constexpr bool both = fm_graph_both<St>;
    const u64 ne = edge_offsets[nnodes];
    const FmEdge *d_final = f->g_edges.as<FmEdge>();
    int rc;
    if (!(flags & DEBWT_FM_GRAPH_ALL_EDGES) && ne) {
        std::vector<u64> len(nnodes);
        for (u64 v = 0; v < nnodes; v++) {
            const u64 r = both ? v / 2 : v;
            len[v] = (r + 1 < f->nrec ? f->rec_starts[r + 1] : f->n) - 1 - f->rec_starts[r];
        }
        FM_ENSURE(f, f->g_len, (size_t)nnodes * 8);
        if constexpr (!both) {                                 // the merge of both strands has left the offsets in g_eoff
            FM_ENSURE(f, f->g_eoff, (size_t)(nnodes + 1) * 8);
            HIPCHK(f, hipMemcpyAsync(f->g_eoff.p, edge_offsets, (nnodes + 1) * 8, hipMemcpyHostToDevice, f->stream));
        }
        HIPCHK(f, hipMemcpyAsync(f->g_len.p, len.data(), nnodes * 8, hipMemcpyHostToDevice, f->stream));
        if ((rc = fm_graph_reduce(f, st, tm, nnodes, f->g_edges.as<FmEdge>(), ne))) return rc;
        std::vector<u32> deg(nnodes);
        FM_ENSURE(f, f->g_deg, (size_t)nnodes * 4);
        tm.begin();
        k_fm_graph_degree<<<grid_for(nnodes, 256), 256, 0, f->stream>>>(f->g_keep.as<u8>(), f->g_eoff.as<u64>(), nnodes, f->g_deg.as<u32>());
        HIPCHK(f, hipMemcpyAsync(deg.data(), f->g_deg.p, nnodes * 4, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_reduce))) return rc;
        for (u64 i = 0; i < nnodes; i++) edge_offsets[i + 1] = edge_offsets[i] + deg[i];
        const u64 nk = edge_offsets[nnodes];
        if (nk != ne - st.reducible) { f->err = std::string(who) + ": the kept edges do not add up"; return DEBWT_EINTERNAL; }
        FM_ENSURE(f, f->g_oseg, (size_t)(nnodes + 1) * 8);
        FM_ENSURE(f, f->g_out, (size_t)std::max<u64>(nk, 1) * sizeof(FmEdge));
        HIPCHK(f, hipMemcpyAsync(f->g_oseg.p, edge_offsets, (nnodes + 1) * 8, hipMemcpyHostToDevice, f->stream));
        tm.begin();
        k_fm_graph_scatter<<<grid_for(ne, 256), 256, 0, f->stream>>>(f->g_edges.as<FmEdge>(), f->g_keep.as<u8>(), f->g_eoff.as<u64>(),
                                                                     f->g_oseg.as<u64>(), nnodes, ne, f->g_out.as<FmEdge>());
        if ((rc = tm.end(&st.ms_reduce))) return rc;
        st.launches += 2;
        d_final = f->g_out.as<FmEdge>();
    }
    const u64 total = edge_offsets[nnodes];
    if (capacity < total || (total && !edges)) {
        f->err = std::string(who) + ": capacity below the edges (edge_offsets[" + (both ? "2 * nrec" : "nrec") + "] = " +
                 std::to_string(total) + ")";
        return DEBWT_ERANGE;
    }
    if (total) {
        HIPCHK(f, hipMemcpyAsync(edges, d_final, (size_t)total * sizeof(FmEdge), hipMemcpyDeviceToHost, f->stream));
        if ((rc = fm_sync(f))) return rc;
    }
    return DEBWT_OK;
}

// Definition 4, and with `both` definition 4b: no link to the source's mirror, none at a self-rc read, and of a unitig and
// its mirror the one with the lower first member.
int fm_unitigs(bool both, const uint8_t *state, const uint64_t *edge_offsets, const debwt_fm_edge *edges, uint64_t nnodes,
               uint64_t *unitig_offsets, uint32_t *members, uint8_t *circular, uint64_t *nunitigs) {
    if (!edge_offsets || !unitig_offsets || !nunitigs || (nnodes && (!state || !members || !circular)) || (nnodes >> 32))
        return DEBWT_EINVAL;
    const u64 e0 = edge_offsets[0];
    for (u64 i = 0; i < nnodes; i++)
        if (edge_offsets[i + 1] < edge_offsets[i]) return DEBWT_EINVAL;
    if (edge_offsets[nnodes] > e0 && !edges) return DEBWT_EINVAL;
    constexpr u32 NONE = 0xFFFFFFFFu;
    std::vector<u32> indeg(nnodes, 0), next(nnodes, NONE);
    for (u64 i = 0; i < nnodes; i++)
        for (u64 e = edge_offsets[i]; e < edge_offsets[i + 1]; e++) {
            if (edges[e].record >= nnodes || state[i] != 0 || state[edges[e].record] != 0) return DEBWT_EINVAL;
            indeg[edges[e].record]++;
        }
    auto selfrc = [&](u64 v) { return state[v & ~1ull] == 0 && state[v | 1] == 1; };   // asked only with `both`: nnodes is even
    std::vector<u8> has_in(nnodes, 0), on_chain(nnodes, 0);
    for (u64 i = 0; i < nnodes; i++)
        if (edge_offsets[i + 1] - edge_offsets[i] == 1) {
            const u32 w = edges[edge_offsets[i]].record;
            if (w != i && indeg[w] == 1 && !(both && (w == (i ^ 1) || selfrc(i) || selfrc(w)))) { next[i] = w; has_in[w] = 1; }
        }
    for (u64 i = 0; i < nnodes; i++)                           // the nodes that a node without an incoming link leads to
        if (state[i] == 0 && !has_in[i])
            for (u64 v = i; v != NONE; v = next[v]) on_chain[v] = 1;
    // every unitig of the link rule in ascending first member; with `both` it stays only when its mirror starts no lower
    u64 nu = 0, nm = 0;
    unitig_offsets[0] = 0;
    for (u64 i = 0; i < nnodes; i++) {
        if (state[i] != 0 || (has_in[i] && on_chain[i])) continue;
        const u64 m0 = nm;
        u64 mirror_first = NONE;
        if (!has_in[i]) {
            u64 last = i;
            for (u64 v = i; v != NONE; v = next[v]) { members[nm++] = (u32)v; last = v; }
            if (both) mirror_first = selfrc(last) ? last : (last ^ 1);
            circular[nu] = 0;
        } else {                                               // the lowest node of a cycle: the ones after it get on_chain
            u64 v = i;
            do { members[nm++] = (u32)v; on_chain[v] = 1; mirror_first = std::min<u64>(mirror_first, v ^ 1); v = next[v]; } while (v != i);
            circular[nu] = 1;
        }
        if (both && mirror_first < i) { nm = m0; continue; }   // the mirror has been, or will be, reported
        unitig_offsets[++nu] = nm;
    }
    *nunitigs = nu;
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_string_graph(debwt_fm *f, uint32_t min_overlap, uint32_t flags, uint8_t *state, uint64_t *edge_offsets,
                                     debwt_fm_edge *edges, uint64_t capacity) {
    if (!f || !state || !edge_offsets) return DEBWT_EINVAL;
    const char *who = "debwt_fm_string_graph";
    const auto t0 = std::chrono::steady_clock::now();
    f->g_stats = debwt_fm_graph_stats{};
    if (!min_overlap) { f->err = "debwt_fm_string_graph: min_overlap must be at least 1"; return DEBWT_EINVAL; }
    if (flags & ~DEBWT_FM_GRAPH_ALL_EDGES) { f->err = "debwt_fm_string_graph: unknown flags"; return DEBWT_EINVAL; }
    if (f->nrec >> 32) { f->err = "debwt_fm_string_graph: 2^32 records or more"; return DEBWT_EINVAL; }
    HIPCHK(f, hipSetDevice(f->device));
    debwt_fm_graph_stats &st = f->g_stats;
    const u64 nrec = f->nrec;
    FmGraphTimer tm(f);
    int rc = tm.init();
    if (rc) return rc;
    if ((rc = fm_graph_found(f, st, who, tm, min_overlap, state, edge_offsets))) return rc;
    st.edges = edge_offsets[nrec];
    st.edge_bytes = edge_offsets[nrec] * sizeof(FmEdge);
    if ((rc = fm_graph_finish(f, st, who, tm, flags, nrec, edge_offsets, edges, capacity))) return rc;
    for (u64 i = 0; i < nrec; i++)                             // record order inside every length group
        for (u64 a = edge_offsets[i]; a < edge_offsets[i + 1];) {
            u64 e = a + 1;
            while (e < edge_offsets[i + 1] && edges[e].length == edges[a].length) e++;
            if (e - a > 1)
                std::sort(edges + a, edges + e, [](const debwt_fm_edge &x, const debwt_fm_edge &y) { return x.record < y.record; });
            a = e;
        }
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_edges_reduce(debwt_fm *f, const uint64_t *reclen, uint64_t nnodes, const uint64_t *edge_offsets,
                                     const debwt_fm_edge *edges, uint8_t *keep) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->g_stats = debwt_fm_graph_stats{};
    auto bad = [&](const std::string &why) { f->err = "debwt_fm_edges_reduce: " + why; return DEBWT_EINVAL; };
    if (!edge_offsets || (nnodes && !reclen)) return bad("a NULL array");
    if (nnodes >> 32) return bad("2^32 nodes or more");
    for (u64 i = 0; i < nnodes; i++)
        if (edge_offsets[i + 1] < edge_offsets[i]) return bad("offsets must not decrease");
    const u64 e0 = edge_offsets[0], ne = edge_offsets[nnodes] - e0;
    if (ne && (!edges || !keep)) return bad("a NULL array");
    std::vector<u64> seen(nnodes, 0);                      // source + 1 of the last list that named the node
    for (u64 i = 0; i < nnodes; i++)
        for (u64 e = edge_offsets[i]; e < edge_offsets[i + 1]; e++) {
            const debwt_fm_edge &x = edges[e];
            const std::string at = "edge " + std::to_string(e) + " of source " + std::to_string(i);
            if (x.record >= nnodes) return bad(at + " names node " + std::to_string(x.record) + " of " + std::to_string(nnodes));
            if (x.record == i) return bad(at + " leads to its own source");
            if (e > edge_offsets[i] && x.length > edges[e - 1].length) return bad(at + " is longer than the one before it");
            if (seen[x.record] == i + 1) return bad(at + " repeats target " + std::to_string(x.record));
            seen[x.record] = i + 1;
            if (x.length >= std::min(reclen[i], reclen[x.record])) return bad(at + " is as long as one of its records");
        }
    debwt_fm_graph_stats &st = f->g_stats;
    st.records = nnodes; st.edges = ne; st.edge_bytes = ne * sizeof(FmEdge);
    if (!ne) return DEBWT_OK;
    HIPCHK(f, hipSetDevice(f->device));
    FmGraphTimer tm(f);
    int rc = tm.init();
    if (rc) return rc;
    std::vector<u64> off(nnodes + 1);
    for (u64 i = 0; i <= nnodes; i++) off[i] = edge_offsets[i] - e0;
    FM_ENSURE(f, f->g_eoff, (size_t)(nnodes + 1) * 8);
    FM_ENSURE(f, f->g_len, (size_t)nnodes * 8);
    if ((rc = fm_graph_reserve(f, "debwt_fm_string_graph", 0, ne))) return rc;
    HIPCHK(f, hipMemcpyAsync(f->g_eoff.p, off.data(), (nnodes + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->g_len.p, reclen, nnodes * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->g_edges.p, edges + e0, (size_t)ne * sizeof(FmEdge), hipMemcpyHostToDevice, f->stream));
    if ((rc = fm_graph_reduce(f, st, tm, nnodes, f->g_edges.as<FmEdge>(), ne))) return rc;
    HIPCHK(f, hipMemcpyAsync(keep + e0, f->g_keep.p, (size_t)ne, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_unitigs(const uint8_t *state, const uint64_t *edge_offsets, const debwt_fm_edge *edges, uint64_t nnodes,
                                uint64_t *unitig_offsets, uint32_t *members, uint8_t *circular, uint64_t *nunitigs) {
    return fm_unitigs(false, state, edge_offsets, edges, nnodes, unitig_offsets, members, circular, nunitigs);
}

extern "C" int debwt_fm_graph_stats_get(const debwt_fm *f, debwt_fm_graph_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->g_stats;
    return DEBWT_OK;
}

// ---- string graph over both strands: what comes between fm_graph_found and fm_graph_finish ---------------------------
// fm_graph_found leaves A in g_edges: ++, +- and -+ of every record.  Here the mirrors of the ++ edges are counted per
// target, the lists of the 2 nrec nodes laid out, every edge placed in its list (b_cat) and ranked into E (g_edges again),
// which leaves every list in (length, target) order.  g_stats is not touched: debwt_fm_graph_stats_get goes on answering
// for the last strand-0 call.

extern "C" int debwt_fm_string_graph_both(debwt_fm *f, uint32_t min_overlap, uint32_t flags, uint8_t *state, uint64_t *edge_offsets,
                                          debwt_fm_edge *edges, uint64_t capacity) {
    if (!f || !state || !edge_offsets) return DEBWT_EINVAL;
    const char *who = "debwt_fm_string_graph_both";
    const auto t0 = std::chrono::steady_clock::now();
    f->b_stats = debwt_fm_graph_both_stats{};
    if (!min_overlap) { f->err = "debwt_fm_string_graph_both: min_overlap must be at least 1"; return DEBWT_EINVAL; }
    if (flags & ~DEBWT_FM_GRAPH_ALL_EDGES) { f->err = "debwt_fm_string_graph_both: unknown flags"; return DEBWT_EINVAL; }
    if (f->nrec >> 31) { f->err = "debwt_fm_string_graph_both: 2^31 records or more"; return DEBWT_EINVAL; }
    HIPCHK(f, hipSetDevice(f->device));
    debwt_fm_graph_both_stats &st = f->b_stats;
    const u64 nrec = f->nrec, nn = 2 * nrec;
    FmGraphTimer tm(f);
    int rc = tm.init();
    if (rc) return rc;
    std::vector<uint64_t> aoff(3 * nrec + 1, 0);
    if ((rc = fm_graph_found(f, st, who, tm, min_overlap, state, aoff.data()))) return rc;
    const u64 na = aoff[3 * nrec];
    std::vector<u32> mm(nrec, 0);
    if (na) {
        FM_ENSURE(f, f->b_aoff, (size_t)(3 * nrec + 1) * 8);
        FM_ENSURE(f, f->b_mm, (size_t)nrec * 4);
        FM_ENSURE(f, f->b_cur, (size_t)nrec * 4);
        HIPCHK(f, hipMemcpyAsync(f->b_aoff.p, aoff.data(), (3 * nrec + 1) * 8, hipMemcpyHostToDevice, f->stream));
        HIPCHK(f, hipMemsetAsync(f->b_mm.p, 0, nrec * 4, f->stream));
        HIPCHK(f, hipMemsetAsync(f->b_cur.p, 0, nrec * 4, f->stream));
        tm.begin();
        k_fm_bigraph_indeg<<<grid_for(na, 256), 256, 0, f->stream>>>(f->g_edges.as<FmEdge>(), f->b_aoff.as<u64>(), nrec, na,
                                                                     f->b_self.as<u8>(), f->b_mm.as<u32>());
        HIPCHK(f, hipMemcpyAsync(mm.data(), f->b_mm.p, nrec * 4, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_merge))) return rc;
        st.launches++;
    }
    edge_offsets[0] = 0;
    for (u64 i = 0; i < nrec; i++) {
        edge_offsets[2 * i + 1] = edge_offsets[2 * i] + (aoff[3 * i + 2] - aoff[3 * i]);
        edge_offsets[2 * i + 2] = edge_offsets[2 * i + 1] + (aoff[3 * i + 3] - aoff[3 * i + 2]) + mm[i];
        st.edges_kind[0] += aoff[3 * i + 1] - aoff[3 * i];
        st.edges_kind[1] += aoff[3 * i + 2] - aoff[3 * i + 1];
        st.edges_kind[2] += aoff[3 * i + 3] - aoff[3 * i + 2];
        st.edges_kind[3] += mm[i];
    }
    const u64 ne = edge_offsets[nn];
    st.edges = ne;
    st.edge_bytes = ne * sizeof(FmEdge);
    FM_ENSURE(f, f->g_eoff, (size_t)(nn + 1) * 8);
    if (ne) {
        FM_ENSURE(f, f->b_cat, (size_t)ne * sizeof(FmEdge));
        HIPCHK(f, hipMemcpyAsync(f->g_eoff.p, edge_offsets, (nn + 1) * 8, hipMemcpyHostToDevice, f->stream));
        tm.begin();
        k_fm_bigraph_place<<<grid_for(na, 256), 256, 0, f->stream>>>(f->g_edges.as<FmEdge>(), f->b_aoff.as<u64>(), nrec, na,
                                                                     f->g_eoff.as<u64>(), f->b_self.as<u8>(), f->b_cur.as<u32>(),
                                                                     f->b_cat.as<FmEdge>());
        if ((rc = tm.end(&st.ms_merge))) return rc;
        if ((rc = fm_graph_reserve(f, who, 0, ne))) return rc; // A has been read: E takes its place
        tm.begin();
        k_fm_bigraph_rank<<<grid_for(ne, 256), 256, 0, f->stream>>>(f->b_cat.as<FmEdge>(), f->g_eoff.as<u64>(), nn, ne,
                                                                    f->g_edges.as<FmEdge>());
        if ((rc = tm.end(&st.ms_merge))) return rc;
        st.launches += 2;
    }
    if ((rc = fm_graph_finish(f, st, who, tm, flags, nn, edge_offsets, edges, capacity))) return rc;
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_unitigs_both(const uint8_t *state, const uint64_t *edge_offsets, const debwt_fm_edge *edges, uint64_t nnodes,
                                     uint64_t *unitig_offsets, uint32_t *members, uint8_t *circular, uint64_t *nunitigs) {
    if (nnodes & 1) return DEBWT_EINVAL;
    return fm_unitigs(true, state, edge_offsets, edges, nnodes, unitig_offsets, members, circular, nunitigs);
}

extern "C" int debwt_fm_graph_both_stats_get(const debwt_fm *f, debwt_fm_graph_both_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->b_stats;
    return DEBWT_OK;
}

// ---- graph cleaning (fm_clean_kernels.h) ----------------------------------------------------------------------------------
// The caller's lists are checked on the host, uploaded once (g_eoff, g_edges) and transposed once; the in-degree counts
// come back for the host to lay the in-lists out.  A round is at most six launches and one copy of the counters, which
// tells the host whether the round removed anything.

extern "C" void debwt_fm_clean_defaults(debwt_fm_clean_opts *o) {
    if (!o) return;
    o->max_tip = 4; o->max_bubble = 16; o->max_rounds = 8; o->flags = 0;
}

extern "C" int debwt_fm_graph_clean(debwt_fm *f, const uint8_t *state, const uint64_t *edge_offsets, const debwt_fm_edge *edges,
                                    uint64_t nnodes, const debwt_fm_clean_opts *opts, uint8_t *state_out, uint8_t *edge_keep) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    f->cl_stats = debwt_fm_clean_stats{};
    auto bad = [&](const std::string &why) { f->err = "debwt_fm_graph_clean: " + why; return DEBWT_EINVAL; };
    if (!opts || !edge_offsets || (nnodes && (!state || !state_out))) return bad("a NULL array");
    const u32 T = opts->max_tip, B = opts->max_bubble, R = opts->max_rounds;
    if (!T && !B) return bad("max_tip and max_bubble are both 0");
    if (!R) return bad("max_rounds must be at least 1");
    if (opts->flags & ~DEBWT_FM_CLEAN_MIRRORED) return bad("unknown flags");
    if (nnodes >> 32) return bad("2^32 nodes or more");
    const bool mirrored = opts->flags & DEBWT_FM_CLEAN_MIRRORED;
    if (mirrored && (nnodes & 1)) return bad("an odd number of nodes with DEBWT_FM_CLEAN_MIRRORED");
    for (u64 i = 0; i < nnodes; i++)
        if (edge_offsets[i + 1] < edge_offsets[i]) return bad("offsets must not decrease");
    const u64 e0 = edge_offsets[0], ne = edge_offsets[nnodes] - e0;
    if (ne && (!edges || !edge_keep)) return bad("a NULL array");
    for (u64 i = 0; i < nnodes; i++)
        for (u64 e = edge_offsets[i]; e < edge_offsets[i + 1]; e++) {
            const u64 t = edges[e].record;
            if (t < nnodes && state[i] == 0 && state[t] == 0) continue;
            const std::string at = "edge " + std::to_string(e) + " of source " + std::to_string(i);
            if (t >= nnodes) return bad(at + " names node " + std::to_string(t) + " of " + std::to_string(nnodes));
            if (state[i] != 0) return bad(at + " leaves a node that is not alive");
            return bad(at + " leads to node " + std::to_string(t) + ", which is not alive");
        }
    debwt_fm_clean_stats &st = f->cl_stats;
    st.nodes = nnodes; st.edges = ne;
    if (nnodes && state_out != state) std::memcpy(state_out, state, nnodes);   /* state_out may be state itself */
    if (!ne) {                                                 // nothing to walk: the one round removes nothing
        st.rounds = 1;
        st.ms_wall = (float)fm_ms_since(t0);
        return DEBWT_OK;
    }
    HIPCHK(f, hipSetDevice(f->device));
    FmGraphTimer tm(f);
    int rc = tm.init();
    if (rc) return rc;
    std::vector<u64> off(nnodes + 1);
    for (u64 i = 0; i <= nnodes; i++) off[i] = edge_offsets[i] - e0;
    FM_ENSURE(f, f->g_eoff, (size_t)(nnodes + 1) * 8);
    FM_ENSURE(f, f->cl_state, (size_t)nnodes);
    FM_ENSURE(f, f->cl_src, (size_t)ne * 4);
    FM_ENSURE(f, f->cl_cnt, (size_t)nnodes * 4);
    FM_ENSURE(f, f->cl_toff, (size_t)(nnodes + 1) * 8);
    FM_ENSURE(f, f->cl_tin, (size_t)ne * 8);
    FM_ENSURE(f, f->cl_snap, (size_t)nnodes * 16);
    FM_ENSURE(f, f->cl_mark, (size_t)ne);
    FM_ENSURE(f, f->cl_ctr, FM_CL_NCTR * 8);
    if ((rc = fm_graph_reserve(f, "debwt_fm_graph_clean", 0, ne))) return rc;
    HIPCHK(f, hipMemcpyAsync(f->g_eoff.p, off.data(), (nnodes + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->g_edges.p, edges + e0, (size_t)ne * sizeof(FmEdge), hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->cl_state.p, state, nnodes, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(f->cl_cnt.p, 0, nnodes * 4, f->stream));
    HIPCHK(f, hipMemsetAsync(f->cl_ctr.p, 0, FM_CL_NCTR * 8, f->stream));
    const u64 *d_eoff = f->g_eoff.as<u64>();
    const FmEdge *d_edges = f->g_edges.as<FmEdge>();
    u8 *d_state = f->cl_state.as<u8>(), *d_mark = f->cl_mark.as<u8>();
    u32 *d_src = f->cl_src.as<u32>(), *d_cnt = f->cl_cnt.as<u32>();
    u64 *d_toff = f->cl_toff.as<u64>(), *d_tin = f->cl_tin.as<u64>(), *d_ctr = f->cl_ctr.as<u64>();
    u32 *d_outdeg = f->cl_snap.as<u32>(), *d_indeg = d_outdeg + nnodes, *d_succ = d_indeg + nnodes, *d_pred = d_succ + nnodes;
    const FmCleanSnap S{d_outdeg, d_indeg, d_succ, d_pred};
    const u32 ge = grid_for(ne, 256), gn = grid_for(nnodes, 256);
    // the transpose: in-degrees on the device, their running sum on the host, the edge numbers into their in-lists
    std::vector<u32> cnt(nnodes);
    tm.begin();
    k_fm_clean_source<<<ge, 256, 0, f->stream>>>(d_eoff, nnodes, d_edges, ne, d_src, d_cnt);
    HIPCHK(f, hipMemcpyAsync(cnt.data(), d_cnt, nnodes * 4, hipMemcpyDeviceToHost, f->stream));
    if ((rc = tm.end(&st.ms_clean))) return rc;
    off[0] = 0;
    for (u64 i = 0; i < nnodes; i++) off[i + 1] = off[i] + cnt[i];
    if (off[nnodes] != ne) { f->err = "debwt_fm_graph_clean: the in-degrees do not add up"; return DEBWT_EINTERNAL; }
    HIPCHK(f, hipMemcpyAsync(d_toff, off.data(), (nnodes + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(d_cnt, 0, nnodes * 4, f->stream));
    tm.begin();
    k_fm_clean_transpose<<<ge, 256, 0, f->stream>>>(d_edges, ne, d_toff, d_cnt, d_tin);
    st.launches += 2;
    u64 h[FM_CL_NCTR] = {};
    for (u32 round = 0; round < R; round++) {
        if (round) tm.begin();
        const u64 before = h[FM_CL_TIP_NODES] + h[FM_CL_BUBBLE_NODES];
        k_fm_clean_degree<<<gn, 256, 0, f->stream>>>(d_eoff, d_edges, d_toff, d_tin, d_src, d_state, nnodes, d_outdeg, d_indeg, d_succ, d_pred);
        st.launches++;
        if (T) {
            k_fm_clean_tip_mark<<<ge, 256, 0, f->stream>>>(d_edges, d_src, ne, d_state, S, T, d_mark, d_ctr);
            k_fm_clean_tip_apply<<<ge, 256, 0, f->stream>>>(d_eoff, d_edges, d_toff, d_tin, d_src, ne, S, T, d_mark, d_state, d_ctr);
            st.launches += 2;
        }
        if (B) {
            if (T) {                                           // the bubble phase reads the graph after the tips have gone
                k_fm_clean_degree<<<gn, 256, 0, f->stream>>>(d_eoff, d_edges, d_toff, d_tin, d_src, d_state, nnodes, d_outdeg, d_indeg, d_succ, d_pred);
                st.launches++;
            }
            k_fm_clean_bubble<<<gn, 256, 0, f->stream>>>(d_eoff, d_edges, d_state, nnodes, S, B, mirrored ? 1u : 0u, d_mark, d_ctr);
            k_fm_clean_bubble_apply<<<ge, 256, 0, f->stream>>>(d_edges, ne, S, B, d_mark, d_state, d_ctr);
            st.launches += 2;
        }
        HIPCHK(f, hipMemcpyAsync(h, d_ctr, sizeof h, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_clean))) return rc;
        st.rounds++;
        if (h[FM_CL_TIP_NODES] + h[FM_CL_BUBBLE_NODES] == before) break;
    }
    st.tips = h[FM_CL_TIPS]; st.tip_nodes = h[FM_CL_TIP_NODES];
    st.bubbles = h[FM_CL_BUBBLES]; st.bubble_nodes = h[FM_CL_BUBBLE_NODES];
    st.steps = h[FM_CL_STEPS];
    HIPCHK(f, hipMemcpyAsync(state_out, d_state, nnodes, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    for (u64 i = 0; i < nnodes; i++)
        for (u64 e = edge_offsets[i]; e < edge_offsets[i + 1]; e++)
            edge_keep[e] = state_out[i] == 0 && state_out[edges[e].record] == 0;
    st.ms_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_edges_compact(const uint64_t *edge_offsets, const debwt_fm_edge *edges, const uint8_t *keep, uint64_t nnodes,
                                      uint64_t *offsets_out, debwt_fm_edge *edges_out) {
    if (!edge_offsets || !offsets_out) return DEBWT_EINVAL;
    for (u64 i = 0; i < nnodes; i++)
        if (edge_offsets[i + 1] < edge_offsets[i]) return DEBWT_EINVAL;
    if (edge_offsets[nnodes] > edge_offsets[0] && (!edges || !keep || !edges_out)) return DEBWT_EINVAL;
    u64 o = 0;
    for (u64 i = 0; i < nnodes; i++) {
        const u64 a = edge_offsets[i], b = edge_offsets[i + 1];    // read before offsets_out[i + 1] is written: in place is fine
        offsets_out[i] = o;
        for (u64 e = a; e < b; e++)
            if (keep[e]) edges_out[o++] = edges[e];
    }
    offsets_out[nnodes] = o;
    return DEBWT_OK;
}

extern "C" int debwt_fm_clean_stats_get(const debwt_fm *f, debwt_fm_clean_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->cl_stats;
    return DEBWT_OK;
}

// ---- pileup, calls and consensus (fm_pile_kernels.h) -----------------------------------------------------------------------
// A call uploads the reads, the alignments and the CIGARs once; the validity pass runs before anything touches the table,
// so a refused call leaves the table as it was.  The table, its window and the separator list stay with the index.

namespace {

static_assert(sizeof(debwt_fm_pile_aln) == sizeof(FmPileAln) && sizeof(debwt_fm_variant) == sizeof(FmPileVar) &&
              sizeof(debwt_fm_ins_event) == sizeof(FmPileIns), "pileup structs of the ABI and of the kernels differ");

// why alignment g breaks definition 7 (the device found that it does)
std::string fm_pile_why(const uint64_t *offsets, u64 npat, const debwt_fm_pile_aln &A, const uint32_t *ops, u64 nops, u64 n) {
    if (A.pattern >= npat) return "pattern " + std::to_string(A.pattern) + " of " + std::to_string(npat);
    if (A.strand > 1) return "strand " + std::to_string(A.strand);
    u64 q = 0, t = 0;
    for (u64 o = 0; o < nops; o++) {
        const u32 kind = ops[o] & 15u, len = ops[o] >> 4;
        if (kind > 2) return "op code " + std::to_string(kind);
        if (!len) return "an op of length 0";
        if ((o == 0 || o + 1 == nops) && kind) return "a CIGAR that does not begin and end with M";
        if (kind != 2) q += len;
        if (kind != 1) t += len;
    }
    if ((u64)A.qbeg + q > offsets[A.pattern + 1] - offsets[A.pattern]) return "query bases past the end of the read";
    if (A.tbeg > n || t > n - A.tbeg) return "text past position n";
    return "nothing";
}

// reads (when given), alignments and CIGARs to the device and through the validity pass: q_off, p_aln, p_coff, p_cig,
// p_span, p_ctr (cleared first; h receives the counters)
int fm_pile_plan(debwt_fm *f, const std::string &who, const uint64_t *offsets, u64 npat, const debwt_fm_pile_aln *alns, u64 naln,
                 const uint64_t *coff, const uint32_t *cigar, FmGraphTimer &tm, float *ms, u64 (&h)[FM_PL_NCTR]) {
    auto bad = [&](const std::string &why) { f->err = who + ": " + why; return DEBWT_EINVAL; };
    if (!offsets || !coff || (naln && !alns)) return bad("a NULL array");
    for (u64 i = 0; i < npat; i++)
        if (offsets[i + 1] < offsets[i]) return bad("offsets must not decrease");
    for (u64 g = 0; g < naln; g++)
        if (coff[g + 1] < coff[g]) return bad("cigar_offsets must not decrease");
    const u64 c0 = coff[0], nops = coff[naln] - c0;
    if (nops && !cigar) return bad("a NULL array");
    for (u64 k = 0; k < FM_PL_NCTR; k++) h[k] = 0;
    h[FM_PL_BAD] = ~0ull;
    FM_ENSURE(f, f->p_ctr, FM_PL_NCTR * 8);
    HIPCHK(f, hipMemcpyAsync(f->p_ctr.p, h, sizeof h, hipMemcpyHostToDevice, f->stream));
    if (!naln) return fm_sync(f);
    std::vector<u64> off(naln + 1);
    for (u64 g = 0; g <= naln; g++) off[g] = coff[g] - c0;
    FM_ENSURE(f, f->q_off, (size_t)(npat + 1) * 8);
    FM_ENSURE(f, f->p_aln, (size_t)naln * sizeof(FmPileAln));
    FM_ENSURE(f, f->p_coff, (size_t)(naln + 1) * 8);
    FM_ENSURE(f, f->p_cig, (size_t)std::max<u64>(nops, 1) * 4);
    FM_ENSURE(f, f->p_span, (size_t)naln * 8);
    std::vector<u64> poff(npat + 1);                           // from 0, like the characters that are uploaded
    for (u64 i = 0; i <= npat; i++) poff[i] = offsets[i] - offsets[0];
    HIPCHK(f, hipMemcpyAsync(f->q_off.p, poff.data(), (npat + 1) * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->p_aln.p, alns, naln * sizeof(FmPileAln), hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemcpyAsync(f->p_coff.p, off.data(), (naln + 1) * 8, hipMemcpyHostToDevice, f->stream));
    if (nops) HIPCHK(f, hipMemcpyAsync(f->p_cig.p, cigar + c0, nops * 4, hipMemcpyHostToDevice, f->stream));
    tm.begin();
    k_fm_pile_plan<<<grid_for(naln, 256), 256, 0, f->stream>>>(f->q_off.as<u64>(), npat, f->p_aln.as<FmPileAln>(), naln,
                                                               f->p_coff.as<u64>(), f->p_cig.as<u32>(), f->n, f->p_span.as<u64>(),
                                                               f->p_ctr.as<u64>());
    HIPCHK(f, hipMemcpyAsync(h, f->p_ctr.p, sizeof h, hipMemcpyDeviceToHost, f->stream));
    int rc = tm.end(ms);
    if (rc) return rc;
    if (h[FM_PL_BAD] != ~0ull) {
        const u64 g = h[FM_PL_BAD];
        if (g >= naln) { f->err = who + ": the validity pass named an alignment that does not exist"; return DEBWT_EINTERNAL; }
        return bad("alignment " + std::to_string(g) + ": " + fm_pile_why(offsets, npat, alns[g], cigar + coff[g], coff[g + 1] - coff[g], f->n));
    }
    return DEBWT_OK;
}

}  // namespace

extern "C" int debwt_fm_pileup(debwt_fm *f, const char *patterns, const uint64_t *offsets, uint64_t npat,
                               const debwt_fm_pile_aln *alns, uint64_t naln, const uint64_t *cigar_offsets, const uint32_t *cigar,
                               uint64_t wbeg, uint64_t wend, uint32_t flags) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    const std::string who = "debwt_fm_pileup";
    auto bad = [&](const std::string &why) { f->err = who + ": " + why; return DEBWT_EINVAL; };
    if (flags & ~DEBWT_FM_PILE_ADD) return bad("unknown flags");
    if (wend <= wbeg || wend > f->n) return bad("the window must be a non-empty part of [0, n)");
    const bool add = (flags & DEBWT_FM_PILE_ADD) && f->has_ptable;
    if (add && (wbeg != f->p_wbeg || wend != f->p_wend)) return bad("DEBWT_FM_PILE_ADD with a window that is not the resident table's");
    if (!offsets) return bad("a NULL array");
    if (offsets[npat] < offsets[0]) return bad("offsets must not decrease");
    const u64 nchars = offsets[npat] - offsets[0];
    if (nchars && !patterns) return bad("a NULL array");
    // the counters of the call before this one stay in p_stats until this one has passed the validity pass
    debwt_fm_pile_stats st{};
    st.call_positions = f->p_stats.call_positions; st.call_variants = f->p_stats.call_variants;
    st.ms_call = f->p_stats.ms_call; st.ms_call_wall = f->p_stats.ms_call_wall;
    HIPCHK(f, hipSetDevice(f->device));
    FmGraphTimer tm(f);
    int rc = tm.init();
    if (rc) return rc;
    u64 h[FM_PL_NCTR];
    if ((rc = fm_pile_plan(f, who, offsets, npat, alns, naln, cigar_offsets, cigar, tm, &st.ms_plan, h))) return rc;
    if (naln) st.launches++;
    const u64 W = wend - wbeg;
    if (W > (~(size_t)0 >> 6)) { f->err = who + ": the window is too large for one table"; return DEBWT_ENOMEM; }
    if (!add) {
        f->has_ptable = false;
        FM_ENSURE(f, f->p_table, (size_t)W * 32);
        HIPCHK(f, hipMemsetAsync(f->p_table.p, 0, (size_t)W * 32, f->stream));
        f->p_wbeg = wbeg; f->p_wend = wend;
        f->has_ptable = true;
    }
    st.alignments = naln; st.ops = h[FM_PL_OPS]; st.m_columns = h[FM_PL_MCOLS]; st.d_bases = h[FM_PL_DBASES]; st.i_ops = h[FM_PL_IOPS];
    st.table_bytes = (u64)W * 32;
    if (naln && st.ops) {
        // the reads as 4-bit codes, staged once for the call; the characters are padded to whole words of 8
        const u64 nwords = (nchars + 7) >> 3;
        FM_ENSURE(f, f->q_chars, (size_t)std::max<u64>(nwords, 1) * 8);
        FM_ENSURE(f, f->p_codes, (size_t)std::max<u64>(nwords, 1) * 4);
        if (nwords) HIPCHK(f, hipMemsetAsync(f->q_chars.as<u8>() + (nwords - 1) * 8, 0, 8, f->stream));
        if (nchars) HIPCHK(f, hipMemcpyAsync(f->q_chars.p, patterns + offsets[0], nchars, hipMemcpyHostToDevice, f->stream));
        const char *form = getenv("DEBWT_PILE_FORM");
        u32 G = st.m_columns / naln >= 256 ? 64 : 16;
        if (form && !strcmp(form, "lane")) G = 1;
        else if (form && !strcmp(form, "group16")) G = 16;
        else if (form && !strcmp(form, "group64")) G = 64;
        else if (form && *form && strcmp(form, "group")) return bad("DEBWT_PILE_FORM must be lane, group, group16 or group64");
        const u32 *d_codes = f->p_codes.as<u32>();
        const u64 *d_off = f->q_off.as<u64>(), *d_coff = f->p_coff.as<u64>(), *d_span = f->p_span.as<u64>();
        const FmPileAln *d_aln = f->p_aln.as<FmPileAln>();
        const u32 *d_cig = f->p_cig.as<u32>();
        u32 *d_tab = f->p_table.as<u32>();
        u64 *d_ctr = f->p_ctr.as<u64>();
        if (grid_for(naln * G, 256) == 0 || naln * G > (u64)0x7FFFFFFF * 256) { f->err = who + ": too many alignments for one call"; return DEBWT_ERANGE; }
        if (nwords) k_fm_pile_stage<<<grid_for(nwords, 256), 256, 0, f->stream>>>(f->q_chars.as<u8>(), nwords, f->p_codes.as<u32>());
        tm.begin();
        const u32 grid = grid_for(naln * G, 256);
        if (G == 1) k_fm_pile_count_lane<<<grid, 256, 0, f->stream>>>(d_codes, d_off, d_aln, naln, d_coff, d_cig, d_span, wbeg, wend, d_tab, d_ctr);
        else if (G == 16) k_fm_pile_count_group<16><<<grid, 256, 0, f->stream>>>(d_codes, d_off, d_aln, naln, d_coff, d_cig, d_span, wbeg, wend, d_tab, d_ctr);
        else k_fm_pile_count_group<64><<<grid, 256, 0, f->stream>>>(d_codes, d_off, d_aln, naln, d_coff, d_cig, d_span, wbeg, wend, d_tab, d_ctr);
        HIPCHK(f, hipMemcpyAsync(h, f->p_ctr.p, sizeof h, hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&st.ms_kernel))) return rc;
        st.launches += nwords ? 2 : 1;
        st.group = G;
        st.ev_base = h[FM_PL_EV_BASE]; st.ev_other = h[FM_PL_EV_OTHER]; st.ev_del = h[FM_PL_EV_DEL]; st.ev_ins = h[FM_PL_EV_INS];
    } else if ((rc = fm_sync(f))) return rc;
    st.ms_wall = (float)fm_ms_since(t0);
    f->p_stats = st;
    return DEBWT_OK;
}

extern "C" int debwt_fm_pile_fetch(debwt_fm *f, uint64_t *window, uint32_t *counts, uint64_t capacity) {
    if (!f || !window) return DEBWT_EINVAL;
    if (!f->has_ptable) { f->err = "debwt_fm_pile_fetch: no table (debwt_fm_pileup)"; return DEBWT_ESTATE; }
    window[0] = f->p_wbeg; window[1] = f->p_wend;
    const u64 W = f->p_wend - f->p_wbeg;
    if (capacity < W) { f->err = "debwt_fm_pile_fetch: capacity below the window"; return DEBWT_ERANGE; }
    if (!counts) return DEBWT_EINVAL;
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipMemcpyAsync(counts, f->p_table.p, (size_t)W * 32, hipMemcpyDeviceToHost, f->stream));
    return fm_sync(f);
}

extern "C" int debwt_fm_pile_release(debwt_fm *f) {
    if (!f) return DEBWT_EINVAL;
    HIPCHK(f, hipSetDevice(f->device));
    HIPCHK(f, hipStreamSynchronize(f->stream));
    if (f->p_table.p) { (void)hipFree(f->p_table.p); f->p_table.p = nullptr; f->p_table.cap = 0; }
    f->has_ptable = false;
    f->p_wbeg = f->p_wend = 0;
    return DEBWT_OK;
}

extern "C" void debwt_fm_pile_defaults(debwt_fm_pile_opts *o) {
    if (!o) return;
    o->min_depth = 4; o->min_permille = 600;
}

extern "C" int debwt_fm_pile_call(debwt_fm *f, const debwt_fm_pile_opts *opts, uint8_t *calls, uint8_t *ref,
                                  debwt_fm_variant *variants, uint64_t capacity, uint64_t *nvars) {
    if (!f) return DEBWT_EINVAL;
    const auto t0 = std::chrono::steady_clock::now();
    if (!calls || !nvars) { f->err = "debwt_fm_pile_call: a NULL array"; return DEBWT_EINVAL; }
    if (!f->has_ptable) { f->err = "debwt_fm_pile_call: no table (debwt_fm_pileup)"; return DEBWT_ESTATE; }
    debwt_fm_pile_opts o;
    debwt_fm_pile_defaults(&o);
    if (opts) o = *opts;
    int rc;
    if (!f->has_text && (rc = debwt_fm_restore_text(f))) return rc;
    HIPCHK(f, hipSetDevice(f->device));
    FmGraphTimer tm(f);
    if ((rc = tm.init())) return rc;
    const u64 wbeg = f->p_wbeg, W = f->p_wend - wbeg, nrec = f->nrec, nblocks = (W + 255) / 256;
    std::vector<u64> sep(nrec);
    for (u64 r = 0; r + 1 < nrec; r++) sep[r] = f->rec_starts[r + 1] - 1;
    sep[nrec - 1] = f->n - 1;
    FM_ENSURE(f, f->p_sep, (size_t)nrec * 8);
    FM_ENSURE(f, f->p_calls, (size_t)W * 2);
    FM_ENSURE(f, f->p_vcnt, (size_t)nblocks * 4);
    FM_ENSURE(f, f->p_vbase, (size_t)nblocks * 8);
    HIPCHK(f, hipMemcpyAsync(f->p_sep.p, sep.data(), nrec * 8, hipMemcpyHostToDevice, f->stream));
    HIPCHK(f, hipMemsetAsync(f->p_vcnt.p, 0, nblocks * 4, f->stream));
    u8 *d_calls = f->p_calls.as<u8>(), *d_ref = d_calls + W;
    std::vector<u32> vcnt(nblocks);
    float ms = 0.f;
    tm.begin();
    k_fm_pile_call<false><<<(u32)nblocks, 256, 0, f->stream>>>(f->p_table.as<u32>(), f->text.as<u64>(), f->p_sep.as<u64>(), nrec, wbeg, W,
                                                              o.min_depth, o.min_permille, d_calls, d_ref, f->p_vcnt.as<u32>(), nullptr, nullptr);
    HIPCHK(f, hipMemcpyAsync(vcnt.data(), f->p_vcnt.p, nblocks * 4, hipMemcpyDeviceToHost, f->stream));
    HIPCHK(f, hipMemcpyAsync(calls, d_calls, W, hipMemcpyDeviceToHost, f->stream));
    if (ref) HIPCHK(f, hipMemcpyAsync(ref, d_ref, W, hipMemcpyDeviceToHost, f->stream));
    if ((rc = tm.end(&ms))) return rc;
    std::vector<u64> vbase(nblocks + 1, 0);
    for (u64 b = 0; b < nblocks; b++) vbase[b + 1] = vbase[b] + vcnt[b];
    const u64 total = vbase[nblocks];
    *nvars = total;
    f->p_stats.call_positions = W; f->p_stats.call_variants = total;
    if (capacity < total) { f->err = "debwt_fm_pile_call: capacity below the number of variants"; return DEBWT_ERANGE; }
    if (total) {
        if (!variants) { f->err = "debwt_fm_pile_call: a NULL array"; return DEBWT_EINVAL; }
        FM_ENSURE(f, f->p_vars, (size_t)total * sizeof(FmPileVar));
        HIPCHK(f, hipMemcpyAsync(f->p_vbase.p, vbase.data(), nblocks * 8, hipMemcpyHostToDevice, f->stream));
        tm.begin();
        k_fm_pile_call<true><<<(u32)nblocks, 256, 0, f->stream>>>(f->p_table.as<u32>(), f->text.as<u64>(), f->p_sep.as<u64>(), nrec, wbeg, W,
                                                                 o.min_depth, o.min_permille, d_calls, d_ref, f->p_vcnt.as<u32>(),
                                                                 f->p_vbase.as<u64>(), f->p_vars.as<FmPileVar>());
        HIPCHK(f, hipMemcpyAsync(variants, f->p_vars.p, total * sizeof(FmPileVar), hipMemcpyDeviceToHost, f->stream));
        if ((rc = tm.end(&ms))) return rc;
    }
    f->p_stats.ms_call = ms;
    f->p_stats.ms_call_wall = (float)fm_ms_since(t0);
    return DEBWT_OK;
}

extern "C" int debwt_fm_pile_insertions(debwt_fm *f, uint64_t npat, const uint64_t *offsets, const debwt_fm_pile_aln *alns,
                                        uint64_t naln, const uint64_t *cigar_offsets, const uint32_t *cigar,
                                        const uint64_t *positions, uint64_t npos, debwt_fm_ins_event *events, uint64_t capacity,
                                        uint64_t *nevents) {
    if (!f) return DEBWT_EINVAL;
    const std::string who = "debwt_fm_pile_insertions";
    auto bad = [&](const std::string &why) { f->err = who + ": " + why; return DEBWT_EINVAL; };
    if (!nevents || (npos && !positions)) return bad("a NULL array");
    for (u64 k = 1; k < npos; k++)
        if (positions[k] <= positions[k - 1]) return bad("positions must ascend strictly");
    HIPCHK(f, hipSetDevice(f->device));
    FmGraphTimer tm(f);
    int rc = tm.init();
    if (rc) return rc;
    u64 h[FM_PL_NCTR];
    float ms = 0.f;
    if ((rc = fm_pile_plan(f, who, offsets, npat, alns, naln, cigar_offsets, cigar, tm, &ms, h))) return rc;
    *nevents = 0;
    if (!naln || !npos || !h[FM_PL_IOPS]) return DEBWT_OK;
    FM_ENSURE(f, f->p_sep, (size_t)npos * 8);                  // the positions; the call kernel uploads its separators anew
    FM_ENSURE(f, f->p_vcnt, (size_t)naln * 4);
    FM_ENSURE(f, f->p_vbase, (size_t)naln * 8);
    HIPCHK(f, hipMemcpyAsync(f->p_sep.p, positions, npos * 8, hipMemcpyHostToDevice, f->stream));
    std::vector<u32> acnt(naln);
    const u32 grid = grid_for(naln, 256);
    k_fm_pile_ins<false><<<grid, 256, 0, f->stream>>>(f->p_aln.as<FmPileAln>(), naln, f->p_coff.as<u64>(), f->p_cig.as<u32>(),
                                                      f->p_span.as<u64>(), f->p_sep.as<u64>(), npos, f->p_vcnt.as<u32>(), nullptr, nullptr);
    HIPCHK(f, hipMemcpyAsync(acnt.data(), f->p_vcnt.p, naln * 4, hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    std::vector<u64> abase(naln + 1, 0);
    for (u64 g = 0; g < naln; g++) abase[g + 1] = abase[g] + acnt[g];
    const u64 total = abase[naln];
    *nevents = total;
    if (capacity < total) { f->err = who + ": capacity below the number of events"; return DEBWT_ERANGE; }
    if (!total) return DEBWT_OK;
    if (!events) return bad("a NULL array");
    FM_ENSURE(f, f->p_vars, (size_t)total * sizeof(FmPileIns));
    HIPCHK(f, hipMemcpyAsync(f->p_vbase.p, abase.data(), naln * 8, hipMemcpyHostToDevice, f->stream));
    k_fm_pile_ins<true><<<grid, 256, 0, f->stream>>>(f->p_aln.as<FmPileAln>(), naln, f->p_coff.as<u64>(), f->p_cig.as<u32>(),
                                                     f->p_span.as<u64>(), f->p_sep.as<u64>(), npos, f->p_vcnt.as<u32>(),
                                                     f->p_vbase.as<u64>(), f->p_vars.as<FmPileIns>());
    HIPCHK(f, hipMemcpyAsync(events, f->p_vars.p, total * sizeof(FmPileIns), hipMemcpyDeviceToHost, f->stream));
    if ((rc = fm_sync(f))) return rc;
    // written in (alignment, op) order; a stable sort by position leaves (t, aln, qpos)
    std::stable_sort(events, events + total, [](const debwt_fm_ins_event &a, const debwt_fm_ins_event &b) { return a.t < b.t; });
    return DEBWT_OK;
}

extern "C" int debwt_fm_ins_vote(const char *patterns, const uint64_t *offsets, uint64_t npat, const debwt_fm_pile_aln *alns,
                                 uint64_t naln, const debwt_fm_ins_event *events, uint64_t nevents, char *out, uint64_t capacity,
                                 uint64_t *len, uint32_t *support) {
    if (!len || !support || (nevents && (!patterns || !offsets || !alns || !events))) return DEBWT_EINVAL;
    std::vector<std::string> strs;
    strs.reserve(nevents);
    for (u64 k = 0; k < nevents; k++) {
        const debwt_fm_ins_event &e = events[k];
        if (e.aln >= naln) return DEBWT_EINVAL;
        const debwt_fm_pile_aln &A = alns[e.aln];
        if (A.pattern >= npat || A.strand > 1) return DEBWT_EINVAL;
        const u64 base = offsets[A.pattern], m = offsets[A.pattern + 1] - base;
        if ((u64)e.qpos + e.len > m) return DEBWT_EINVAL;
        std::string s(e.len, 'N');
        for (u32 x = 0; x < e.len; x++) {
            const u64 i = (u64)e.qpos + x;
            const char ch = patterns[base + (A.strand ? m - 1 - i : i)];
            const char *hit = strchr("ACGT", ch & ~0x20);
            if (ch && hit) s[x] = A.strand ? "TGCA"[hit - "ACGT"] : *hit;
        }
        strs.push_back(std::move(s));
    }
    // equal strings side by side, shorter first, then in lexicographic order: the first run of the largest size wins
    std::sort(strs.begin(), strs.end(), [](const std::string &a, const std::string &b) {
        return a.size() != b.size() ? a.size() < b.size() : a < b;
    });
    u64 best = 0, best_n = 0;
    for (u64 i = 0; i < strs.size();) {
        u64 j = i;
        while (j < strs.size() && strs[j] == strs[i]) j++;
        if (j - i > best_n) { best = i; best_n = j - i; }
        i = j;
    }
    *support = (uint32_t)best_n;
    *len = best_n ? strs[best].size() : 0;
    if (capacity < *len) return DEBWT_ERANGE;
    if (*len) {
        if (!out) return DEBWT_EINVAL;
        memcpy(out, strs[best].data(), *len);
    }
    return DEBWT_OK;
}

extern "C" int debwt_fm_consensus(const uint8_t *ref, const uint8_t *calls, uint64_t wbeg, uint64_t wend, const uint64_t *ins_t,
                                  const uint64_t *ins_offsets, const char *ins_bases, const uint32_t *ins_support,
                                  const uint32_t *ins_depth, uint64_t nins, uint32_t min_permille, const uint64_t *rec_starts,
                                  uint64_t nrec, uint64_t n, uint64_t *out_offsets, char *out, uint64_t capacity) {
    if (!ref || !calls || !rec_starts || !out_offsets || wend <= wbeg || wend > n || !nrec) return DEBWT_EINVAL;
    if (nins && (!ins_t || !ins_offsets || !ins_support || !ins_depth)) return DEBWT_EINVAL;
    for (u64 k = 1; k < nins; k++)
        if (ins_t[k] <= ins_t[k - 1]) return DEBWT_EINVAL;
    for (u64 k = 0; k < nins; k++)
        if (ins_offsets[k + 1] < ins_offsets[k] || (ins_offsets[k + 1] > ins_offsets[k] && !ins_bases)) return DEBWT_EINVAL;
    // two passes over the same walk: the lengths, then the letters
    for (int pass = 0; pass < 2; pass++) {
        u64 o = 0, k = 0;
        for (u64 r = 0; r < nrec; r++) {
            const u64 rs = rec_starts[r], re = (r + 1 < nrec ? rec_starts[r + 1] : n) - 1;   // the record's bases: [rs, re)
            if (re < rs || re >= n) return DEBWT_EINVAL;
            if (!pass) out_offsets[r] = o;
            for (u64 t = std::max<u64>(rs, wbeg); t < std::min<u64>(re, wend); t++) {
                const u32 c = calls[t - wbeg], b = c & 15u, rf = ref[t - wbeg];
                if (b < 4) { if (pass) out[o] = "ACGT"[b]; o++; }
                else if (b == 5 && rf < 4) { if (pass) out[o] = "acgt"[rf]; o++; }
                if (!(c & 0x10u)) continue;
                while (k < nins && ins_t[k] < t) k++;
                if (k < nins && ins_t[k] == t && (u64)ins_support[k] * 1000 >= (u64)min_permille * ins_depth[k]) {
                    const u64 L = ins_offsets[k + 1] - ins_offsets[k];
                    if (pass) memcpy(out + o, ins_bases + ins_offsets[k], L);
                    o += L;
                }
            }
        }
        if (!pass) {
            out_offsets[nrec] = o;
            if (capacity < o) return DEBWT_ERANGE;
            if (o && !out) return DEBWT_EINVAL;
        }
    }
    return DEBWT_OK;
}

extern "C" int debwt_fm_pile_stats_get(const debwt_fm *f, debwt_fm_pile_stats *out) {
    if (!f || !out) return DEBWT_EINVAL;
    *out = f->p_stats;
    return DEBWT_OK;
}

extern "C" void debwt_fm_destroy(debwt_fm *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (DevBuf *b : {&f->idx, &f->rowlists, &f->sa, &f->q_chars, &f->q_off, &f->q_out, &f->q_runs, &f->s_hits, &f->s_ctr,
                      &f->s_plist, &f->m_slot, &f->m_cnt, &f->m_obase, &f->m_spans, &f->m_ranges, &f->m_cspans,
                      &f->m_cranges, &f->text, &f->x_jobs, &f->x_best, &f->x_cells, &f->x_flags, &f->x_tr, &f->x_cigoff,
                      &f->x_cig, &f->x_anchors, &f->o_table, &f->o_slot, &f->o_runs, &f->o_nruns, &f->o_nhits, &f->o_rbase,
                      &f->o_hbase, &f->o_cruns, &f->o_rout, &f->o_hits, &f->anchors, &f->e_jobs, &f->e_seg, &f->e_out, &f->e_ctr,
                      &f->e_sep, &f->k_table, &f->k_coff, &f->k_counts, &f->k_ctr, &f->k_active, &f->k_info, &f->k_ntr,
                      &f->k_trials, &f->k_trun, &f->k_res, &f->sp_front, &f->sp_codes, &f->sp_mults, &f->sp_ctr, &f->sp_hist,
                      &f->sp_gsum, &f->g_coff, &f->g_state, &f->g_hbase, &f->g_raw, &f->g_flag,
                      &f->g_deg, &f->g_oseg, &f->g_edges, &f->g_eoff, &f->g_len, &f->g_keep, &f->g_out, &f->g_ctr, &f->b_state,
                      &f->b_self, &f->b_row, &f->b_cnt, &f->b_whb, &f->b_rawbase, &f->b_tbase, &f->b_pos, &f->b_aoff, &f->b_mm,
                      &f->b_cur, &f->b_cat, &f->b_ctr, &f->cl_state, &f->cl_src, &f->cl_cnt, &f->cl_toff, &f->cl_tin, &f->cl_snap,
                      &f->cl_mark, &f->cl_ctr, &f->p_table, &f->p_codes, &f->p_aln, &f->p_coff, &f->p_cig, &f->p_span, &f->p_ctr,
                      &f->p_sep, &f->p_calls, &f->p_vcnt, &f->p_vbase, &f->p_vars, &f->esa_lcp, &f->esa_sa, &f->esa_da, &f->rec_P})
        if (b->p) (void)hipFree(b->p);
    for (DevBuf &b : f->s_items)
        if (b.p) (void)hipFree(b.p);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}
